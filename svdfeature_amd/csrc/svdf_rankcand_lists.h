// svdf_rankcand_lists.h -- the host-only part of the candidate lists of svdf_rank_eval*_cand / svdf_rank_topn_cand:
// their validation, a section's ranked set (the distinct candidate ids, ascending, with the section's positives among them), the index of
// every positive inside that set, the cut of a piece at the entry budget and the tile table the score kernel walks.  Plain C++ without a
// device call, so that tools/check_rankcand_lists.cpp can run it under a sanitizer.
#ifndef SVDF_RANKCAND_LISTS_H_
#define SVDF_RANKCAND_LISTS_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

constexpr int RANK_CAND_TILE = 64;   // most (section, candidate) pairs of one tile: one per lane of the wave that scores it

// Everything the _cand calls refuse about the candidate lists themselves; `who` is the prefix of the messages, "rank_eval" or "rank_topn".
// Section s carries the ids cand_item[cand_ptr[s] .. cand_ptr[s + 1]); an id must be below num_item (the ranker's message, bare).  Empty
// lists and repeated ids are legal.
static inline void rank_cand_validate(const char *who, long S, const int64_t *cand_ptr, const unsigned *cand_item, long num_item) {
    const std::string w(who);
    if (S <= 0) return;
    if (!cand_ptr) fail(w + ": cand_ptr is missing");
    if (cand_ptr[0] < 0) fail(w + ": cand_ptr must start at >= 0");
    for (long s = 0; s < S; s++)
        if (cand_ptr[s + 1] < cand_ptr[s]) fail(w + ": cand_ptr must not decrease");
    if (cand_ptr[S] != 0 && !cand_item) fail(w + ": cand_item is missing");
    for (int64_t j = cand_ptr[0]; j < cand_ptr[S]; j++)
        if ((long)cand_item[j] >= num_item) fail("sample item index exceed bound");
}

struct RankCandLists {
    std::vector<int> ranked;      // [S] size of section s's ranked set
    std::vector<int64_t> first;   // [S + 1] the ranked set of a KEPT section s: ids[first[s] .. first[s + 1]), distinct, ascending
    std::vector<int> ids;
    std::vector<int64_t> pos_at;  // [pos_ptr[S] - pos_ptr[0]] positive j of section s is ids[pos_at[j - pos_ptr[0]]]
};

// The sections [a, b) of rank_cand_build: ranked[s], the size of a kept section's set in first[s + 1] (summed up by the caller), the index of
// every positive INSIDE its section's set in pos_at, and the sets themselves appended to `ids`.
static inline void rank_cand_build_range(long a, long b, const int64_t *cand_ptr, const unsigned *cand_item, const int64_t *pos_ptr, const unsigned *pos_item,
                                         long num_item, RankCandLists &out, std::vector<int> &ids) {
    std::vector<unsigned> set, pos;
    std::vector<uint64_t> mark(((size_t)num_item + 63) / 64, 0);   // one bit per item, all clear between sections
    for (long s = a; s < b; s++) {
        set.assign(cand_item + (cand_ptr[s + 1] > cand_ptr[s] ? cand_ptr[s] : 0), cand_item + (cand_ptr[s + 1] > cand_ptr[s] ? cand_ptr[s + 1] : 0));
        pos.clear();
        if (pos_ptr) {
            pos.assign(pos_item + (pos_ptr[s + 1] > pos_ptr[s] ? pos_ptr[s] : 0), pos_item + (pos_ptr[s + 1] > pos_ptr[s] ? pos_ptr[s + 1] : 0));
            for (unsigned p : pos)
                if ((long)p >= num_item) fail("sample item index exceed bound");
            std::sort(pos.begin(), pos.end());
            if (std::adjacent_find(pos.begin(), pos.end()) != pos.end()) fail("rank_eval: a positive item is repeated inside a section");
            set.insert(set.end(), pos.begin(), pos.end());   // a positive is a candidate by definition; listed as well it counts once
        }
        if (!set.empty() && set.size() * 8 >= mark.size()) {
            // a long list: mark its ids and read the marks back in order -- sorted and distinct in one pass over n ids and num_item / 64 words
            size_t lo = mark.size(), hi = 0;
            for (unsigned c : set) {
                const size_t w = (size_t)c >> 6;
                mark[w] |= (uint64_t)1 << (c & 63);
                lo = std::min(lo, w);
                hi = std::max(hi, w);
            }
            set.clear();
            for (size_t w = lo; w <= hi; w++) {
                uint64_t m = mark[w];
                mark[w] = 0;
                for (; m; m &= m - 1) set.push_back((unsigned)(w << 6) + (unsigned)__builtin_ctzll(m));
            }
        } else {
            std::sort(set.begin(), set.end());
            set.erase(std::unique(set.begin(), set.end()), set.end());
        }
        out.ranked[(size_t)s] = (int)set.size();
        out.first[(size_t)s + 1] = 0;
        if (!pos_ptr || !pos.empty()) {
            out.first[(size_t)s + 1] = (int64_t)set.size();
            ids.insert(ids.end(), set.begin(), set.end());
            if (pos_ptr)
                for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++)
                    out.pos_at[(size_t)(j - pos_ptr[0])] = std::lower_bound(set.begin(), set.end(), pos_item[j]) - set.begin();
        }
    }
}

// The ranked sets of validated lists.  pos_ptr == nullptr (a top-N call): the distinct candidates, every section kept.  Else (a positions
// call; pos_ptr has been checked to start at >= 0 and not to decrease): the distinct candidates and positives together, and only the
// sections WITH positives are kept -- the others get their size and no ids, nothing of them is scored.  Refuses a positive that is out of
// bound or repeated inside its section.  threads > 1: contiguous ranges of sections with about equal numbers of entries are built side by
// side and joined in order; the result, and the refusal where several sections earn one, are those of one thread.
static inline void rank_cand_build(long S, const int64_t *cand_ptr, const unsigned *cand_item, const int64_t *pos_ptr, const unsigned *pos_item,
                                   long num_item, RankCandLists &out, int threads = 1) {
    out.ranked.assign((size_t)std::max<long>(S, 0), 0);
    out.first.assign((size_t)std::max<long>(S, 0) + 1, 0);
    out.ids.clear();
    out.pos_at.clear();
    if (S <= 0) return;
    if (pos_ptr) out.pos_at.assign((size_t)(pos_ptr[S] - pos_ptr[0]), 0);
    const int T = (int)std::max<long>(1, std::min<long>(threads, S));
    if (T == 1) {
        out.ids.reserve((size_t)(cand_ptr[S] - cand_ptr[0]) + out.pos_at.size());
        rank_cand_build_range(0, S, cand_ptr, cand_item, pos_ptr, pos_item, num_item, out, out.ids);
    } else {
        std::vector<long> cut((size_t)T + 1, S);   // range t: sections [cut[t], cut[t + 1]), about 1 / T of the entries (a section counts as one more)
        cut[0] = 0;
        const int64_t total = cand_ptr[S] - cand_ptr[0] + S;
        for (int t = 1; t < T; t++) {
            long lo = cut[(size_t)t - 1], hi = S;
            while (lo < hi) {
                const long m = lo + (hi - lo) / 2;
                if (cand_ptr[m] - cand_ptr[0] + m < total * t / T) lo = m + 1; else hi = m;
            }
            cut[(size_t)t] = lo;
        }
        std::vector<std::vector<int>> part((size_t)T);
        std::vector<std::string> error((size_t)T);
        std::vector<char> failed((size_t)T, 0);
        std::vector<std::thread> th;
        for (int t = 0; t < T; t++)
            th.emplace_back([&, t] {
                try {
                    part[(size_t)t].reserve((size_t)(cand_ptr[cut[(size_t)t + 1]] - cand_ptr[cut[(size_t)t]]) +
                                            (pos_ptr ? (size_t)(pos_ptr[cut[(size_t)t + 1]] - pos_ptr[cut[(size_t)t]]) : 0));
                    rank_cand_build_range(cut[(size_t)t], cut[(size_t)t + 1], cand_ptr, cand_item, pos_ptr, pos_item, num_item, out, part[(size_t)t]);
                } catch (const std::exception &e) {
                    failed[(size_t)t] = 1;
                    error[(size_t)t] = e.what();
                }
            });
        for (std::thread &x : th) x.join();
        for (int t = 0; t < T; t++)
            if (failed[(size_t)t]) fail(error[(size_t)t]);   // the first range that failed holds the first section that fails
        size_t n = 0;
        for (const std::vector<int> &p : part) n += p.size();
        out.ids.reserve(n);
        for (const std::vector<int> &p : part) out.ids.insert(out.ids.end(), p.begin(), p.end());
    }
    for (long s = 0; s < S; s++) {   // sizes -> offsets; a positive's index inside its set -> its index in ids
        out.first[(size_t)s + 1] += out.first[(size_t)s];
        if (pos_ptr)
            for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) out.pos_at[(size_t)(j - pos_ptr[0])] += out.first[(size_t)s];
    }
}

// The piece that starts at section s0: whole sections whose entries -- per section its pairs, one word, and what `extra` names (positives,
// feedback and line entries; nullptr: none) -- stay within `budget`; a section larger than the budget is a piece of its own.  A piece holds
// fewer than 2^29 pairs unless one section alone has more, which is refused.  Returns its end.
static inline long rank_cand_piece(const char *who, long s0, long S, const std::vector<int64_t> &first, const int64_t *const *extra, int num_extra,
                                   int64_t budget) {
    if (budget > ((int64_t)1 << 29) - 1) budget = ((int64_t)1 << 29) - 1;
    long e = s0;
    int64_t load = 0;
    while (e < S) {
        int64_t add = first[(size_t)e + 1] - first[(size_t)e] + 1;
        for (int x = 0; x < num_extra; x++)
            if (extra[x]) add += extra[x][e + 1] - extra[x][e];
        if (e > s0 && load + add > budget) break;
        load += add;
        e++;
    }
    if (first[(size_t)e] - first[(size_t)s0] >= (int64_t)1 << 29) fail(std::string(who) + ": one section with more than 2^29 candidates");
    return e;
}

// The tile table of the sections [s0, s1): tile t holds the pairs [tile_q0[t], tile_q0[t + 1]) of the piece (pair q is ids[first[s0] + q]),
// at most RANK_CAND_TILE consecutive ones, all of section s0 + tile_sec[t]: a tile never crosses a section.  A section without pairs has no tile.
static inline void rank_cand_tiles(long s0, long s1, const std::vector<int64_t> &first, std::vector<int> &tile_q0, std::vector<int> &tile_sec) {
    tile_q0.clear();
    tile_sec.clear();
    const int64_t base = first[(size_t)s0];
    for (long s = s0; s < s1; s++)
        for (int64_t q = first[(size_t)s]; q < first[(size_t)s + 1]; q += RANK_CAND_TILE) {
            tile_q0.push_back((int)(q - base));
            tile_sec.push_back((int)(s - s0));
        }
    tile_q0.push_back((int)(first[(size_t)s1] - base));
}

}  // namespace svdf
#endif

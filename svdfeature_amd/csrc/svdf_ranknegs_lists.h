// svdf_ranknegs_lists.h -- the host-only part of svdf_rank_negatives / svdf_rank_eval*_sampled: the rule that
// draws a section's negatives (stated in full in include/svdfeature_amd.h), the validation of bans and positives in the words of
// svdf_rank_eval_positions, a section's excluded ids (distinct, ascending), the availability rule, and the pair offsets of the sections, which
// follow from SIZES alone.  Plain C++ without a device call, so that tools/check_ranknegs_lists.cpp can run it under a sanitizer; the two
// functions of the rule are also what k_rank_negs_draw computes with.
#ifndef SVDF_RANKNEGS_LISTS_H_
#define SVDF_RANKNEGS_LISTS_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#ifdef __HIPCC__
#define SVDF_RANK_NEGS_HD __host__ __device__
#else
#define SVDF_RANK_NEGS_HD
#endif

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

constexpr int RANK_NEGS_MAX = 4096;                        // largest num_neg: the draw kernel's table of 2 * num_neg slots stays within 32 KiB of LDS
constexpr uint64_t RANK_NEGS_G = 0x9E3779B97F4A7C15ull;    // splitmix64's increment

// splitmix64's output function; everything wraps mod 2^64
SVDF_RANK_NEGS_HD static inline uint64_t rank_negs_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the stream of section s, s being the section's index IN THE CALL
SVDF_RANK_NEGS_HD static inline uint64_t rank_negs_stream(uint64_t seed, uint64_t s) { return rank_negs_mix(seed + (s + 1) * RANK_NEGS_G); }
// draw t = 0, 1, 2, .. of a stream: the high word of the mixed counter, mapped onto [0, num_item) by multiply-high
SVDF_RANK_NEGS_HD static inline unsigned rank_negs_draw(uint64_t stream, uint64_t t, unsigned num_item) {
    return (unsigned)(((rank_negs_mix(stream + (t + 1) * RANK_NEGS_G) >> 32) * (uint64_t)num_item) >> 32);
}

struct RankNegsLists {
    std::vector<int> ranked;         // [S] npos_s + num_neg (num_neg for a section without positives)
    std::vector<int64_t> ex_first;   // [S + 1] the excluded ids of a section WITH positives: ex_ids[ex_first[s] .. ex_first[s + 1]), distinct, ascending
    std::vector<int> ex_ids;
    std::vector<int64_t> first;      // [S + 1] the pairs of a section with positives: npos_s + num_neg of them, the positives first; others have none
};

// The sections [a, b) of rank_negs_build: the bans and positives validated as svdf_rank_eval_positions validates them (its stamp pass, its
// messages, its order inside a section), the availability rule, ranked[s], and -- as SIZES, summed up by the caller -- the excluded ids of a
// section with positives in ex_first[s + 1] and its pairs in first[s + 1]; the excluded lists themselves are appended to `ids`.
static inline void rank_negs_build_range(long a, long b, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                                         long num_item, int num_neg, RankNegsLists &out, std::vector<int> &ids) {
    std::vector<long> stamp((size_t)num_item, 0);   // 2 (s - a) + 1: banned in section s, 2 (s - a) + 2: positive of section s
    for (long s = a; s < b; s++) {
        const bool keep = pos_ptr[s + 1] > pos_ptr[s];
        const long banned = 2 * (s - a) + 1, positive = banned + 1;
        const size_t at = ids.size();
        if (ban_ptr)
            for (int64_t j = ban_ptr[s]; j < ban_ptr[s + 1]; j++) {
                const unsigned id = ban_item[j];
                if ((long)id >= num_item) fail("sample item index exceed bound");
                if (stamp[id] == banned) continue;   // a repeated ban counts once
                stamp[id] = banned;
                if (keep) ids.push_back((int)id);
            }
        for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {
            const unsigned id = pos_item[j];
            if ((long)id >= num_item) fail("sample item index exceed bound");
            if (stamp[id] == banned) fail("each pos sample item can not occur in baned sample list");
            if (stamp[id] == positive) fail("rank_eval: a positive item is repeated inside a section");
            stamp[id] = positive;
            ids.push_back((int)id);
        }
        std::sort(ids.begin() + (long)at, ids.end());
        out.ex_first[(size_t)s + 1] = (int64_t)(ids.size() - at);
        out.first[(size_t)s + 1] = 0;
        if (!keep) continue;
        const int64_t npos = pos_ptr[s + 1] - pos_ptr[s], avail = (int64_t)num_item - (int64_t)(ids.size() - at);
        if (avail < 2 * (int64_t)num_neg || avail * 64 < (int64_t)num_item)
            fail("rank_eval: section " + std::to_string(s) + " leaves " + std::to_string(avail) + " items to draw " + std::to_string(num_neg) +
                 " negatives from " + std::to_string(num_item) + "; list its candidates instead (svdf_rank_eval_positions_cand)");
        out.ranked[(size_t)s] = (int)(npos + num_neg);   // npos <= num_item - 2 * num_neg
        out.first[(size_t)s + 1] = npos + num_neg;
    }
}

// Everything the sampled calls refuse about num_neg, the positives and the bans, then the lists; ban_ptr == nullptr: no bans.  A section with
// positives must leave avail = num_item - |excluded| ids with avail >= 2 * num_neg and avail * 64 >= num_item, so that a draw is accepted
// with probability >= 1 / 128 whatever has been drawn: the expected draws of a section are bounded by 128 * num_neg.  threads > 1:
// contiguous ranges of sections with about equal numbers of entries are built side by side and joined in order, as rank_cand_build does;
// the result, and the refusal where several sections earn one, are those of one thread.
static inline void rank_negs_build(long S, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, long num_item,
                                   int num_neg, RankNegsLists &out, int threads = 1) {
    if (num_neg < 1 || num_neg > RANK_NEGS_MAX) fail("rank_eval: num_neg must be between 1 and 4096");
    if (S < 0 || (S > 0 && !pos_ptr) || num_item < 1 || num_item > 0x7fffffffL) fail("rank_eval: bad arguments");
    out.ranked.assign((size_t)S, num_neg);
    out.ex_first.assign((size_t)S + 1, 0);
    out.first.assign((size_t)S + 1, 0);
    out.ex_ids.clear();
    if (S == 0) return;
    if (pos_ptr[0] < 0) fail("rank_eval: pos_ptr must start at >= 0");
    if (ban_ptr && ban_ptr[0] < 0) fail("rank_eval: ban_ptr must start at >= 0");
    for (long s = 0; s < S; s++) {
        if (pos_ptr[s + 1] < pos_ptr[s]) fail("rank_eval: pos_ptr must not decrease");
        if (ban_ptr && ban_ptr[s + 1] < ban_ptr[s]) fail("rank_eval: ban_ptr must not decrease");
    }
    if (pos_ptr[S] != 0 && !pos_item) fail("rank_eval: pos_item is missing");
    if (ban_ptr && ban_ptr[S] != 0 && !ban_item) fail("rank_eval: ban_item is missing");
    const int T = (int)std::max<long>(1, std::min<long>(threads, S));
    if (T == 1) {
        rank_negs_build_range(0, S, pos_ptr, pos_item, ban_ptr, ban_item, num_item, num_neg, out, out.ex_ids);
    } else {
        auto entries = [&](long s) { return pos_ptr[s] - pos_ptr[0] + (ban_ptr ? ban_ptr[s] - ban_ptr[0] : 0) + s; };   // (a section counts as one more)
        std::vector<long> cut((size_t)T + 1, S);
        cut[0] = 0;
        for (int t = 1; t < T; t++) {
            long lo = cut[(size_t)t - 1], hi = S;
            while (lo < hi) {
                const long m = lo + (hi - lo) / 2;
                if (entries(m) < entries(S) * t / T) lo = m + 1; else hi = m;
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
                    rank_negs_build_range(cut[(size_t)t], cut[(size_t)t + 1], pos_ptr, pos_item, ban_ptr, ban_item, num_item, num_neg, out, part[(size_t)t]);
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
        out.ex_ids.reserve(n);
        for (const std::vector<int> &p : part) out.ex_ids.insert(out.ex_ids.end(), p.begin(), p.end());
    }
    for (long s = 0; s < S; s++) {   // sizes -> offsets
        out.ex_first[(size_t)s + 1] += out.ex_first[(size_t)s];
        out.first[(size_t)s + 1] += out.first[(size_t)s];
    }
}

// The negatives of one section by the sequential definition: the first num_neg ids of draw(0), draw(1), .. that are neither in `ex` (the
// section's excluded ids) nor earlier in the sequence, in the order of the sequence.  `mark` holds one clear bit per item and is clear again
// on return.  Returns the number of draws taken.
static inline uint64_t rank_negs_section(uint64_t stream, unsigned num_item, const int *ex, size_t nex, int num_neg, int *neg, std::vector<uint64_t> &mark) {
    for (size_t j = 0; j < nex; j++) mark[(size_t)ex[j] >> 6] |= (uint64_t)1 << (ex[j] & 63);
    uint64_t t = 0;
    for (int have = 0; have < num_neg; t++) {
        const unsigned id = rank_negs_draw(stream, t, num_item);
        uint64_t &w = mark[(size_t)id >> 6];
        const uint64_t bit = (uint64_t)1 << (id & 63);
        if (w & bit) continue;
        w |= bit;
        neg[have++] = (int)id;
    }
    for (size_t j = 0; j < nex; j++) mark[(size_t)ex[j] >> 6] = 0;
    for (int j = 0; j < num_neg; j++) mark[(size_t)neg[j] >> 6] = 0;
    return t;
}

// svdf_rank_negatives: neg_out[S][num_neg], row s the negatives of section s in draw order, -1 for a section without positives
static inline void rank_negs_host(long S, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, long num_item,
                                  int num_neg, uint64_t seed, int *neg_out) {
    RankNegsLists L;
    rank_negs_build(S, pos_ptr, pos_item, ban_ptr, ban_item, num_item, num_neg, L);
    if (S > 0 && !neg_out) fail("rank_eval: bad arguments");
    std::vector<uint64_t> mark(((size_t)num_item + 63) / 64, 0);
    for (long s = 0; s < S; s++) {
        int *row = neg_out + (size_t)s * (size_t)num_neg;
        if (pos_ptr[s + 1] == pos_ptr[s]) { std::fill(row, row + num_neg, -1); continue; }
        rank_negs_section(rank_negs_stream(seed, (uint64_t)s), (unsigned)num_item, L.ex_ids.data() + L.ex_first[(size_t)s],
                          (size_t)(L.ex_first[(size_t)s + 1] - L.ex_first[(size_t)s]), num_neg, row, mark);
    }
}

// slots of the draw kernel's table of seen ids: the next power of two >= 2 * num_neg (2 .. 8192), so that it is never more than half full
static inline int rank_negs_table(int num_neg) {
    int n = 2;
    while (n < 2 * num_neg) n <<= 1;
    return n;
}

}  // namespace svdf
#endif

// svdf_ranktopn_lists.h -- the host-only part of svdf_rank_topn: validation of the caller's lists and the cut into
// pieces of whole sections.  Plain C++ without a device call, so that tools/check_ranktopn_lists.cpp can run it under a sanitizer.
#ifndef SVDF_RANKTOPN_LISTS_H_
#define SVDF_RANKTOPN_LISTS_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

struct RankTopnLists {
    std::vector<int64_t> ban_first;   // [S + 1] the distinct banned ids of section s: ban_ids[ban_first[s] .. ban_first[s + 1]), ascending
    std::vector<int> ban_ids;
    std::vector<int> count;           // [S] min(top_n, num_item - distinct banned ids)
};

// Everything svdf_rank_topn refuses about its lists, in the ranker's words where the ranker has them; nothing is written before all of it holds.
static inline void rank_topn_validate(long S, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, long num_user, long num_item,
                                      int top_n, RankTopnLists &out) {
    auto need = [](bool ok, const char *msg) { if (!ok) fail(msg); };
    need(S >= 0 && (S == 0 || user), "rank_topn: bad arguments");
    out.ban_first.assign((size_t)S + 1, 0);
    out.ban_ids.clear();
    out.count.assign((size_t)S, 0);
    if (S == 0) return;
    if (ban_ptr) {
        need(ban_ptr[0] >= 0, "rank_topn: ban_ptr must start at >= 0");
        for (long s = 0; s < S; s++) need(ban_ptr[s + 1] >= ban_ptr[s], "rank_topn: ban_ptr must not decrease");
        need(ban_ptr[S] == 0 || ban_item, "rank_topn: ban_item is missing");
    }
    std::vector<long> stamp((size_t)num_item, 0);   // s + 1: banned in section s
    for (long s = 0; s < S; s++) {
        need((long)user[s] < num_user, "user feature index exceed bound");
        const size_t first = out.ban_ids.size();
        if (ban_ptr)
            for (int64_t j = ban_ptr[s]; j < ban_ptr[s + 1]; j++) {
                const unsigned b = ban_item[j];
                need((long)b < num_item, "sample item index exceed bound");
                if (stamp[b] == s + 1) continue;   // the ranker's tag write is idempotent
                stamp[b] = s + 1;
                out.ban_ids.push_back((int)b);
            }
        std::sort(out.ban_ids.begin() + (long)first, out.ban_ids.end());
        out.ban_first[(size_t)s + 1] = (int64_t)out.ban_ids.size();
        out.count[(size_t)s] = (int)std::min<long>(top_n, num_item - (long)(out.ban_ids.size() - first));
    }
}

// The piece that starts at section s0: whole sections, at most max_lists of them (one list per section fits the workspace then), whole
// tiles of 64 where more than one tile fits, and fewer than 2^31 banned ids.  Returns its end.
static inline long rank_topn_piece(long s0, long S, long max_lists, const std::vector<int64_t> &ban_first) {
    long n = std::min(S - s0, std::max<long>(1, max_lists));
    if (n > 64 && n < S - s0) n -= n % 64;
    while (n > 1 && ban_first[(size_t)(s0 + n)] - ban_first[(size_t)s0] >= (int64_t)1 << 30) n = (n + 1) / 2;
    return s0 + n;
}

}  // namespace svdf
#endif

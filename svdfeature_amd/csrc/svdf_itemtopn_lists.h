// svdf_itemtopn_lists.h -- the host-only part of svdf_item_topn: validation of the caller's lists, the merge of a
// section's query item into its sorted ban list, and the unit rows of the cosine metric on the host (svdf_item_unit_rows).  The rule is
// stated in full in include/svdfeature_amd.h.  Plain C++ without a device call -- build with -ffp-contract=off, as svdf_pairhard_lists.h:
// every multiply, add, square root and divide below is rounded on its own.
#ifndef SVDF_ITEMTOPN_LISTS_H_
#define SVDF_ITEMTOPN_LISTS_H_

#include <cmath>

#include "svdf_ranktopn_lists.h"

namespace svdf {

// Everything svdf_item_topn refuses about its lists; nothing is written before all of it holds.  Section s excludes the distinct ids of
// its ban list and its own query item[s]: out.ban_ids holds them merged, ascending, the way the sweeps read a ban list.
static inline void item_topn_validate(long S, const unsigned *item, const int64_t *ban_ptr, const unsigned *ban_item, long num_item, int top_n,
                                      RankTopnLists &out) {
    auto need = [](bool ok, const char *msg) { if (!ok) fail(msg); };
    need(S >= 0 && (S == 0 || item), "item_topn: bad arguments");
    out.ban_first.assign((size_t)S + 1, 0);
    out.ban_ids.clear();
    out.count.assign((size_t)S, 0);
    if (S == 0) return;
    if (ban_ptr) {
        need(ban_ptr[0] >= 0, "item_topn: ban_ptr must start at >= 0");
        for (long s = 0; s < S; s++) need(ban_ptr[s + 1] >= ban_ptr[s], "item_topn: ban_ptr must not decrease");
        need(ban_ptr[S] == 0 || ban_item, "item_topn: ban_item is missing");
    }
    std::vector<long> stamp((size_t)num_item, 0);   // s + 1: excluded in section s
    for (long s = 0; s < S; s++) {
        need((long)item[s] < num_item, "sample item index exceed bound");
        const size_t first = out.ban_ids.size();
        stamp[item[s]] = s + 1;                     // the query is always excluded; listing it among its own bans changes nothing
        out.ban_ids.push_back((int)item[s]);
        if (ban_ptr)
            for (int64_t j = ban_ptr[s]; j < ban_ptr[s + 1]; j++) {
                const unsigned b = ban_item[j];
                need((long)b < num_item, "sample item index exceed bound");
                if (stamp[b] == s + 1) continue;
                stamp[b] = s + 1;
                out.ban_ids.push_back((int)b);
            }
        std::sort(out.ban_ids.begin() + (long)first, out.ban_ids.end());
        out.ban_first[(size_t)s + 1] = (int64_t)out.ban_ids.size();
        out.count[(size_t)s] = (int)std::min<long>(top_n, num_item - (long)(out.ban_ids.size() - first));
    }
}

// <p, p> in the pinned order of svdf_rank_topn's score: four serial chains over the 4-float chunks, each started as 0 + product,
// (a0 + a2) + (a1 + a3), the scalar tail in index order
static inline float item_sum_squares(int k, const float *p) {
    const int nfull = k >> 2, ntail = k & 3;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int j = 0; j < nfull; j++) {
        a0 = a0 + p[4 * j] * p[4 * j]; a1 = a1 + p[4 * j + 1] * p[4 * j + 1];
        a2 = a2 + p[4 * j + 2] * p[4 * j + 2]; a3 = a3 + p[4 * j + 3] * p[4 * j + 3];
    }
    float sum = (a0 + a2) + (a1 + a3);
    for (int t = 0; t < ntail; t++) sum = sum + p[4 * nfull + t] * p[4 * nfull + t];
    return sum;
}

// svdf_item_unit_rows: out[r][j] = rows[r][j] / sqrt(<rows[r], rows[r]>), a division per element; a row whose sum of squares is 0 gives +0
static inline void item_unit_rows(long num_row, int num_factor, const float *rows, float *out) {
    if (num_row < 0 || num_factor < 1 || (num_row > 0 && (!rows || !out))) fail("item_unit_rows: bad arguments");
    for (long r = 0; r < num_row; r++) {
        const float *p = rows + (size_t)r * (size_t)num_factor;
        float *o = out + (size_t)r * (size_t)num_factor;
        const float ss = item_sum_squares(num_factor, p);
        const volatile float n = std::sqrt(ss);   // (volatile: the divisions below stay divisions by n, whatever the optimiser is told)
        for (int j = 0; j < num_factor; j++) o[j] = ss == 0.0f ? 0.0f : p[j] / n;
    }
}

}  // namespace svdf
#endif

// svdf_itemtopn.cpp -- similar-item lists on the live model: the host side of svdf_item_topn (refusals, the lists
// through svdf_itemtopn_lists.h, the item side prepared by svdf_k_itemrows.hip) in front of the selecting sweeps of svdf_rank_topn, whose
// body it shares (Engine::rank_topn_sweeps, svdf_ranktopn.cpp).
#include <svdfeature_amd.h>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_itemtopn_lists.h"

namespace svdf {

void Engine::item_topn(long S, const unsigned *item, int metric, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out,
                       float *score_out, int *count_out, int *nan_out) {
    // ---- the configuration: what the _fb calls admit (W_item is one table on a user-group trainer too, and no feedback list is involved),
    // less a feature_item table; a feature_user table does not touch an item row
    if (name_feat_item_ != "NULL")
        fail("item_topn: a feature_item side table changes an item's effective row (its children's rows are added) and is not covered");
    rank_live_refusals("item_topn", true, true);
    check(metric == SVDF_ITEM_DOT || metric == SVDF_ITEM_COSINE, "item_topn: metric must be 0 (SVDF_ITEM_DOT) or 1 (SVDF_ITEM_COSINE)");
    check(top_n >= 1 && top_n <= RANK_TOPN_MAX, "item_topn: top_n must be between 1 and 256");
    // ---- the lists, before any device work
    check(S == 0 || (item_out && count_out && nan_out), "item_topn: bad arguments");
    RankTopnLists L;
    item_topn_validate(S, item, ban_ptr, ban_item, (long)mp_.num_item, top_n, L);
    if (S == 0) return;   // nothing to list: no device is asked for
    need_device("item_topn");
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    // ---- the item side of the sweeps, once per call and never kept: the model may have moved since the last one.  Cosine: the unit rows
    // [num_item][pitch] on both sides; dot: W_item where it lies.  Either way a zero vector [num_item] stands in for i_bias.
    const size_t ni = (size_t)mp_.num_item, nrow = metric == SVDF_ITEM_COSINE ? ni * (size_t)P.pitch : 0;
    try {
        rk_items_.reserve(nrow + ni);
    } catch (const std::exception &e) {
        fail("item_topn: the item side of " + std::to_string((nrow + ni) * sizeof(float)) + " bytes could not be allocated: " + e.what());
    }
    float *unit = rk_items_.p, *zero_bias = rk_items_.p + nrow;
    HIPCHECK(hipMemsetAsync(zero_bias, 0, ni * sizeof(float), stream_));
    const float *item_rows = nullptr;
    const float *base = P.W + (size_t)P.item_off * (size_t)P.pitch;
    if (metric == SVDF_ITEM_COSINE) {
        launch_item_unit_rows(P, unit, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_++;
        item_rows = base = unit;
    }
    rank_topn_sweeps("item_topn", S, item, L, nullptr, nullptr, nullptr, nullptr, item_rows, zero_bias, base, top_n, item_out, score_out, count_out, nan_out);
}

}  // namespace svdf

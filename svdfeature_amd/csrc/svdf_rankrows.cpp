// svdf_rankrows.cpp -- what the live-model ranking calls (svdf_rankeval.cpp, svdf_ranktopn.cpp, svdf_itemtopn.cpp, svdf_rankcand.cpp,
// svdf_ranknegs.cpp; DESIGN.md sections 6w - 6al) share on the host about their sections' rows: how a piece's feedback lists and USER
// lines reach the device and become its effective user rows (svdf_k_rankrows.hip, svdf_k_itemrows.hip), the item side's envelope of a
// prefilter call, and the way a piece's positions go back to the caller.  The lists themselves: svdf_rankrows_lists.h.
#include <svdfeature_amd.h>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankrows_lists.h"

namespace svdf {

// what a call refuses about its feedback lists, its lines and the trainer's tables, on the host
void Engine::rank_rows_validate(const char *who, long S, const RankRowSource &R) {
    if (R.fb.ptr) rank_list_validate(RANK_FB_LISTS, who, S, R.fb, std::min<long>(mp_.num_ufeedback, num_fb_rows()));
    if (!R.lines.ptr && !R.by_lines) return;
    rank_list_validate(RANK_USER_LINES, who, S, R.lines, (long)mp_.num_user);
    rank_lines_check_children(who, "feature_user", feat_user_.index, (long)mp_.num_user);
    rank_lines_check_children(who, "feature_item", feat_item_.index, (long)mp_.num_item);
}

// The tail of a piece's upload: [fb_p0 | fb_index | fb_value] [ul_p0 | ul_index | ul_value], appended to `in` (whose reserve has counted
// rank_rows_words, so that nothing already there moves).
RankRowsAt Engine::rank_rows_pack(const RankRowSource &R, long s0, long s1, std::vector<int> &in) {
    RankRowsAt at;
    auto put = [&](const RankList &L) {
        const size_t o = in.size();
        in.resize(o + rank_list_words(s0, s1, L));
        rank_list_pack(s0, s1, L, in.data() + o);
        return o;
    };
    if (R.fb.ptr) at.fb = put(R.fb);
    if (R.lines.ptr) at.ul = put(R.lines);
    return at;
}

// The effective user rows of the piece [s0, s1), one more launch ahead of its scores: built from the feedback lists and USER lines that
// rank_rows_pack put at `at` of the upload whose device copy is `base`, or -- an item call -- gathered from R.query_base by the sections'
// query items.  Returns the [nsec][pitch] workspace, or nullptr where the sections score with their W_user rows.
const float *Engine::rank_rows_launch(const char *who, const RankRowSource &R, const int *base, const RankRowsAt &at, const unsigned *sec_user,
                                      long s0, long s1) {
    if (!R.fb.ptr && !R.lines.ptr && !R.query_base) return nullptr;
    const DevParams &P = params();
    const size_t nsec = (size_t)(s1 - s0);
    reserve_or_fail(who, rk_rows_, nsec * (size_t)P.pitch, "the user rows of a piece");
    if (R.fb.ptr || R.lines.ptr) {
        RankLiveRowsDev Rows;
        Rows.nsec = (int)nsec; Rows.sec_user = sec_user;
        Rows.fb_p0 = nullptr; Rows.fb_index = nullptr; Rows.fb_value = nullptr;
        if (R.fb.ptr) {
            const size_t nfb = (size_t)(R.fb.ptr[s1] - R.fb.ptr[s0]);
            Rows.fb_p0 = base + at.fb;
            Rows.fb_index = reinterpret_cast<const unsigned *>(base + at.fb + nsec + 1);
            Rows.fb_value = reinterpret_cast<const float *>(base + at.fb + nsec + 1 + nfb);
        }
        if (R.lines.ptr) {
            const size_t nul = (size_t)(R.lines.ptr[s1] - R.lines.ptr[s0]);
            Rows.ul_p0 = base + at.ul;
            Rows.ul_index = reinterpret_cast<const unsigned *>(base + at.ul + nsec + 1);
            Rows.ul_value = reinterpret_cast<const float *>(base + at.ul + nsec + 1 + nul);
        }
        Rows.rows = rk_rows_.p;
        launch_rank_live_rows(P, Rows, stream_);
    } else {
        launch_item_query_rows(P, R.query_base, sec_user, (int)nsec, rk_rows_.p, stream_);
    }
    HIPCHECK(hipGetLastError());
    n_launches_++;
    return rk_rows_.p;
}

// the envelope of the item side a prefilter call scores with, once, ahead of its first piece
void Engine::rank_item_envelope(const char *who, const RankRowSource &R) {
    reserve_or_fail(who, tn_env_, RANK_ENV_WORDS, "the item side's envelope");
    HIPCHECK(hipMemsetAsync(tn_env_.p, 0, RANK_ENV_WORDS * sizeof(unsigned), stream_));
    launch_rank_item_envelope(params(), R.item_rows, R.item_bias, tn_env_.p, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
}

void Engine::rank_sections_counted(const RankRowSource &R, long n) {
    n_rank_eval_sections_ += n;
    if (R.fb.ptr) n_rank_fb_sections_ += n;
    if (R.lines.ptr) n_rank_line_sections_ += n;
}

// A piece's results into the caller's arrays: position[q], tied[q] of positive pos_ptr[s0] + q and nan[s - s0] of every section [s0, s1)
// WITH positives, which counts under 38 / 40 / 41; a section without positives keeps what validation wrote.  Returns how many sections
// were counted: the caller adds them to the counter of its own path.
long Engine::rank_positions_back(const RankRowSource &R, const int64_t *pos_ptr, long s0, long s1, const int *position, const int *tied,
                                 const int *nan, int *position_out, int *tied_out, int *nan_out) {
    long counted = 0;
    for (long s = s0; s < s1; s++) {
        if (pos_ptr[s + 1] == pos_ptr[s]) continue;
        nan_out[s] = nan[s - s0] != 0 ? 1 : 0;
        std::copy(position + (pos_ptr[s] - pos_ptr[s0]), position + (pos_ptr[s + 1] - pos_ptr[s0]), position_out + pos_ptr[s]);
        std::copy(tied + (pos_ptr[s] - pos_ptr[s0]), tied + (pos_ptr[s + 1] - pos_ptr[s0]), tied_out + pos_ptr[s]);
        counted++;
    }
    rank_sections_counted(R, counted);
    return counted;
}

}  // namespace svdf

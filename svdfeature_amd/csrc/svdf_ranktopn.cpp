// svdf_ranktopn.cpp -- top-N item lists on the live model: the host side of svdf_rank_topn (refusals, the lists
// through svdf_ranktopn_lists.h, pieces, the workspace of the selecting sweep in svdf_k_ranktopn.hip).
#include <svdfeature_amd.h>

#include <cstring>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankrows_lists.h"
#include "svdf_ranktopn_lists.h"

namespace svdf {

// what the batch ranking calls on the live model do not cover (svdf_ranker_* does); `who` is the prefix of the messages
void Engine::rank_live_refusals(const char *who, bool svdpp_ok, bool tables_ok) {
    const std::string w(who);
    // (svdpp_ok: the _fb calls, which also take user-group trainers of extend_type 0 / 1 -- both SVDPPFeature with one model, apex_svd.cpp:38-40)
    if (!((!user_group() && mtype_.extend_type == 0) || (svdpp_ok && user_group() && mtype_.extend_type <= 1)))
        fail(w + ": user-group trainers (format_type = 1) and extend_type != 0 are not covered: the score has a feedback part; rank the saved model with svdf_ranker_*");
    // (tables_ok: the _lines calls, whose rows and item side are built with the tables)
    if (!tables_ok && !(name_feat_user_ == "NULL" && name_feat_item_ == "NULL"))
        fail(w + ": feature_user / feature_item side tables change the score and are not covered; rank the saved model with svdf_ranker_*");
    if (mp_.common_latent_space != 0) fail(w + ": common_latent_space != 0 is not covered; rank the saved model with svdf_ranker_*");
    if (!(gpus_ == 1 && !multi_)) fail(w + ": amd:gpus > 1 is not covered (the model is spread over the ranks); rank the saved model with svdf_ranker_*");
    if (!(!is_peer_ && !ipc_ && !rccl_))
        fail(w + ": a rank handle of the one-process-per-GPU exchange holds a partition in flight; rank the saved model with svdf_ranker_*");
    if (!(space_allocated_ && trainer_ready_)) fail(w + ": call init_model / load_model and init_trainer first");
}

// The _fb calls: what rank_live_refusals refuses, except user-group trainers of extend_type 0 / 1, which must bring
// feedback lists; a format_type = 0 trainer must not.  Returns whether the sections' rows are built from feedback lists.
bool Engine::rank_live_fb_refusals(const char *who, bool has_lists, bool tables_ok) {
    rank_live_refusals(who, true, tables_ok);
    const std::string w(who);
    if (!user_group()) {
        if (has_lists) fail(w + ": feedback lists need a user-group trainer (format_type = 1)");
        return false;
    }
    if (!has_lists)
        fail(w + ": fb_ptr is NULL on a user-group trainer; a section without feedback must be given explicitly as an empty list "
                 "(fb_ptr[s] == fb_ptr[s + 1]): the score has a feedback part");
    return true;
}

// top_n of a top-N call: 1 .. 256, and up to 4096 under the knob rank_topn_deep; `tail` ends the message of today's bound
void Engine::rank_topn_admit(const char *who, int top_n, const char *tail) {
    const std::string w(who);
    if (!rank_topn_deep_ && !(top_n >= 1 && top_n <= RANK_TOPN_MAX)) fail(w + ": top_n must be between 1 and 256" + tail);
    if (!(top_n >= 1 && top_n <= RANK_TOPN_DEEP_MAX))
        fail(w + ": top_n must be between 1 and 4096 (knob rank_topn_deep = 1); for longer lists rank the saved model with svdf_ranker_* and top_k");
}

void Engine::rank_topn(long S, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out,
                       int *count_out, int *nan_out) {
    rank_live_refusals("rank_topn");
    RankRowSource R;
    R.user = user;
    rank_topn_run(S, R, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
}

void Engine::rank_topn_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                          const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    RankRowSource R;
    R.user = user;
    if (rank_live_fb_refusals("rank_topn", fb_ptr != nullptr)) R.fb = RankList{fb_ptr, fb_index, fb_value};
    rank_topn_run(S, R, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
}

// The _lines calls: what the _fb calls cover, with or without side tables, every section bringing a USER line.
void Engine::rank_topn_lines(long S, const RankList &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                             const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    RankRowSource R;   // no users: the rows come from the lines
    R.lines = U; R.by_lines = true;
    if (rank_live_fb_refusals("rank_topn", fb_ptr != nullptr, true)) R.fb = RankList{fb_ptr, fb_index, fb_value};
    rank_topn_run(S, R, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
}

// The item side of a _lines call: the model's own (nullptr) or, where a feature_item table is set, the matrix and bias vector that one
// launch of k_rank_live_items prepares on the trainer's stream ahead of the sweeps.
void Engine::rank_live_items(const char *who, RankRowSource &R) {
    R.item_rows = R.item_bias = nullptr;
    if (feat_item_.num_row() == 0) return;
    const DevParams &P = params();
    reserve_or_fail(who, rk_items_, (size_t)mp_.num_item * ((size_t)P.pitch + 1), "the prepared item matrix");
    launch_rank_live_items(P, rk_items_.p, rk_items_.p + (size_t)mp_.num_item * (size_t)P.pitch, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
    R.item_rows = rk_items_.p;
    R.item_bias = rk_items_.p + (size_t)mp_.num_item * (size_t)P.pitch;
}

// R.fb given: the sections score with the rows k_rank_live_rows builds from their feedback lists (the configuration has been admitted);
// R.lines given: from their USER lines, behind the feedback sum where there is one
void Engine::rank_topn_run(long S, RankRowSource R, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out,
                           int *count_out, int *nan_out) {
    rank_topn_admit("rank_topn", top_n, "; for longer lists rank the saved model with svdf_ranker_* and top_k");
    // ---- the lists, before any device work
    check(S == 0 || (item_out && count_out && nan_out), "rank_topn: bad arguments");
    RankTopnLists L;
    rank_topn_validate(S, R.user, ban_ptr, ban_item, (long)mp_.num_user, (long)mp_.num_item, top_n, L, R.by_lines);
    rank_rows_validate("rank_topn", S, R);
    need_device("rank_topn");
    if (S == 0) return;
    flush();   // behind whatever has been staged
    if (R.lines.ptr) rank_live_items("rank_topn", R);   // once per call
    rank_topn_sweeps("rank_topn", S, R, L, top_n, item_out, score_out, count_out, nan_out);
}

// The body the top-N calls share from the upload of the validated lists onward.  R.user is the user of each section, or -- R.query_base
// given, svdf_item_topn (svdf_itemtopn.cpp) -- its query item.  Under the knob rank_topn_prefilter (and rank_topn_scores = 0; DESIGN.md
// section 6ai) the sections go through the matrix sweep and the pinned re-score first; those the rule does not certify are gathered --
// ids, validated ban lists, feedback lists, USER lines -- into contiguous copies, listed once more by the pinned sweeps and scattered to
// their places.  Either way every section's list is the pinned one.
void Engine::rank_topn_sweeps(const char *who, long S, const RankRowSource &R, const RankTopnLists &L, int top_n, int *item_out, float *score_out,
                              int *count_out, int *nan_out) {
    if (!(rank_topn_prefilter_ && !rank_topn_scores_) || top_n > RANK_TOPN_MAX) {   // (the prefilter's M = top_n + slack <= 384 is its design: a deep call goes without)
        rank_topn_pass(who, S, R, L, top_n, item_out, score_out, count_out, nan_out, rank_topn_scores_, nullptr, true);
        return;
    }
    rank_item_envelope(who, R);
    std::vector<int> certified((size_t)S, 0);
    rank_topn_pass(who, S, R, L, top_n, item_out, score_out, count_out, nan_out, 2, certified.data(), true);
    std::vector<long> again;
    for (long s = 0; s < S; s++)
        if (!certified[(size_t)s]) again.push_back(s);
    const long A = (long)again.size();
    n_rank_certified_sections_ += S - A;
    n_rank_relisted_sections_ += A;
    if (A == 0) return;
    // ---- the sections left: contiguous copies of what they bring, the pinned sweeps, the results back to their places
    const long N = top_n;
    const RankRelist X(again, R, L.ban_first, L.ban_ids);
    RankTopnLists LA;
    LA.ban_first = X.ban_first;
    LA.ban_ids = X.ban_ids;
    for (long s : again) LA.count.push_back(L.count[(size_t)s]);
    std::vector<int> a_item((size_t)(A * N)), a_count((size_t)A), a_nan((size_t)A);
    std::vector<float> a_score(score_out ? (size_t)(A * N) : 0);
    rank_topn_pass(who, A, X.rows, LA, top_n, a_item.data(), score_out ? a_score.data() : nullptr, a_count.data(), a_nan.data(), 0, nullptr, false);
    auto one = [](long i) { return i; };
    auto list = [N](long i) { return i * N; };
    X.scatter(a_item.data(), list, item_out, list);
    if (score_out) X.scatter(a_score.data(), list, score_out, list);
    X.scatter(a_count.data(), one, count_out, one);
    X.scatter(a_nan.data(), one, nan_out, one);
}

// One pass over all S sections: pieces, geometry, workspace, the launches, the copy-back and the count check.  An item call's query rows
// are gathered from the [num_item][pitch] matrix R.query_base into the piece's row workspace by one more launch.
void Engine::rank_topn_pass(const char *who, long S, const RankRowSource &R, const RankTopnLists &L, int top_n, int *item_out, float *score_out,
                            int *count_out, int *nan_out, int mode, int *certified, bool counted) {
    const DevParams &P = params();
    // under the prefilter the sweep keeps `keep` = top_n + slack keys per list, and the cap, the geometry and the pieces follow it
    // a deep call (section 6al; never under the prefilter): the deep cap, hence fewer item ranges and more pieces, and the deep launchers
    const int N = top_n, matrix = mode != 0, keep = mode == 2 ? N + rank_topn_slack_ : N, deep = N > RANK_TOPN_MAX;
    const int cap = deep ? rank_topn_deep_cap(N) : rank_topn_cap(P, keep, matrix);
    const long max_lists = std::max<long>(1, rank_topn_budget_ / cap);
    std::vector<int> in, back;
    for (long s0 = 0; s0 < S;) {
        long s1 = rank_topn_piece(s0, S, max_lists, L.ban_first);
        if (R.fb.ptr) s1 = rank_list_piece(RANK_FB_LISTS, who, s0, s1, R.fb, rank_eval_budget_);   // ... and at most rank_eval_budget feedback entries
        if (R.lines.ptr) s1 = rank_list_piece(RANK_USER_LINES, who, s0, s1, R.lines, rank_eval_budget_);   // ... and as many line entries
        const long nsec = s1 - s0;
        const int64_t nban = L.ban_first[(size_t)s1] - L.ban_first[(size_t)s0];
        RankTopnDev D;
        D.nsec = (int)nsec; D.top_n = keep; D.cap = cap; D.matrix = matrix; D.deep = deep;
        rank_topn_geometry(P, nsec, max_lists, &D.gy, &D.items_per_block, matrix);
        // ---- one upload: sec_user | ban_p0 | ban_item [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        const size_t o_user = 0, o_bp0 = (size_t)nsec, o_ban = 2 * (size_t)nsec + 1;
        in.clear();
        in.reserve(o_ban + (size_t)nban + rank_rows_words(R, s0, s1));
        in.resize(o_ban + (size_t)nban);
        for (long s = s0; s < s1; s++) {
            in[o_user + (size_t)(s - s0)] = R.user_of(s);
            in[o_bp0 + (size_t)(s - s0)] = (int)(L.ban_first[(size_t)s] - L.ban_first[(size_t)s0]);
        }
        in[o_bp0 + (size_t)nsec] = (int)nban;
        std::copy(L.ban_ids.begin() + (long)L.ban_first[(size_t)s0], L.ban_ids.begin() + (long)L.ban_first[(size_t)s1], in.begin() + (long)o_ban);
        const RankRowsAt o_rows = rank_rows_pack(R, s0, s1, in);
        reserve_or_fail(who, tn_in_, in.size(), "the lists of a piece");
        tn_in_.upload(in.data(), in.size(), stream_);
        // ---- the workspace: list_cnt | nan_cnt | count | certified | items | scores, and the lists
        const size_t nlist = (size_t)nsec * (size_t)D.gy, nres = (size_t)nsec * (3 + 2 * (size_t)N);
        reserve_or_fail(who, tn_out_, nlist + nres, "the results of a piece");
        reserve_or_fail(who, tn_list_, nlist * (size_t)cap, "the list workspace of a piece");
        HIPCHECK(hipMemsetAsync(tn_out_.p, 0, (nlist + (size_t)nsec) * sizeof(int), stream_));
        D.sec_user = reinterpret_cast<const unsigned *>(tn_in_.p + o_user);
        D.ban_p0 = tn_in_.p + o_bp0; D.ban_item = tn_in_.p + o_ban;
        D.item_rows = R.item_rows; D.item_bias = R.item_bias;
        D.user_rows = rank_rows_launch(who, R, tn_in_.p, o_rows, D.sec_user, s0, s1);
        if (counted && R.fb.ptr) n_rank_fb_sections_ += nsec;
        if (counted && R.lines.ptr) n_rank_line_sections_ += nsec;
        D.list = tn_list_.p;
        D.list_cnt = tn_out_.p; D.nan_cnt = tn_out_.p + nlist; D.count_out = D.nan_cnt + nsec; D.certified = D.count_out + nsec; D.item_out = D.certified + nsec;
        D.score_out = reinterpret_cast<float *>(D.item_out + (size_t)nsec * N);
        if (mode == 2) { D.exact_n = N; D.envelope = tn_env_.p; }
        launch_rank_topn(P, D, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_ += 2;
        // the merge has written the lists as the caller gets them (-1 / 0 beyond a section's count, all of a flagged section): they go
        // straight into the caller's arrays
        back.resize(3 * (size_t)nsec);
        HIPCHECK(hipMemcpyAsync(back.data(), D.nan_cnt, (mode == 2 ? 3 : 2) * (size_t)nsec * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(item_out + (size_t)s0 * N, D.item_out, (size_t)nsec * N * sizeof(int), hipMemcpyDeviceToHost, stream_));
        if (score_out) HIPCHECK(hipMemcpyAsync(score_out + (size_t)s0 * N, D.score_out, (size_t)nsec * N * sizeof(float), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        const int *b_nan = back.data(), *b_cnt = b_nan + nsec, *b_cert = b_cnt + nsec;
        for (long s = s0; s < s1; s++) {
            const size_t q = (size_t)(s - s0);
            if (certified && !(certified[s] = b_cert[q])) continue;   // the pinned sweep lists it, and is checked then
            const bool bad = b_nan[q] != 0;
            if (b_cnt[q] != (bad ? 0 : L.count[(size_t)s])) fail(std::string(who) + ": internal error: a section's list is not as long as its candidates allow");
            nan_out[s] = bad ? 1 : 0;
            count_out[s] = b_cnt[q];
        }
        if (counted) (R.query_base ? n_item_topn_sections_ : n_rank_topn_sections_) += nsec;
        if (mode == 1) n_rank_matrix_sections_ += nsec;
        if (deep) n_rank_deep_sections_ += nsec;
        s0 = s1;
    }
}

}  // namespace svdf

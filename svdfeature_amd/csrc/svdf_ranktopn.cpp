// svdf_ranktopn.cpp -- top-N item lists on the live model: the host side of svdf_rank_topn (refusals, the lists
// through svdf_ranktopn_lists.h, pieces, the workspace of the selecting sweep in svdf_k_ranktopn.hip).
#include <svdfeature_amd.h>

#include <cstring>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankfb_lists.h"
#include "svdf_ranklines_lists.h"
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

void Engine::rank_topn(long S, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out,
                       int *count_out, int *nan_out) {
    rank_live_refusals("rank_topn");
    rank_topn_run(S, user, nullptr, nullptr, nullptr, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
}

void Engine::rank_topn_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                          const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    if (!rank_live_fb_refusals("rank_topn", fb_ptr != nullptr)) fb_ptr = nullptr;
    rank_topn_run(S, user, fb_ptr, fb_index, fb_value, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
}

// The _lines calls: what the _fb calls cover, with or without side tables, every section bringing a USER line.
void Engine::rank_topn_lines(long S, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                             const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    if (!rank_live_fb_refusals("rank_topn", fb_ptr != nullptr, true)) fb_ptr = nullptr;
    const std::vector<unsigned> user((size_t)std::max<long>(S, 1), 0u);   // not read by the kernels: the rows come from the lines
    rank_topn_run(S, user.data(), fb_ptr, fb_index, fb_value, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out, &U);
}

// what a _lines call refuses about its lines and the trainer's tables, on the host
void Engine::rank_lines_admit(const char *who, long S, const RankLines &U) {
    rank_lines_validate(who, S, U, (long)mp_.num_user);
    rank_lines_check_children(who, "feature_user", feat_user_.index, (long)mp_.num_user);
    rank_lines_check_children(who, "feature_item", feat_item_.index, (long)mp_.num_item);
}

// The item side of a _lines call: the model's own (nullptr) or, where a feature_item table is set, the matrix and bias vector that one
// launch of k_rank_live_items prepares on the trainer's stream ahead of the sweeps.
void Engine::rank_live_items(const char *who, const float **item_rows, const float **item_bias) {
    *item_rows = *item_bias = nullptr;
    if (feat_item_.num_row() == 0) return;
    const DevParams &P = params();
    const size_t n = (size_t)mp_.num_item * ((size_t)P.pitch + 1);
    try {
        rk_items_.reserve(n);
    } catch (const std::exception &e) {
        fail(std::string(who) + ": the prepared item matrix of " + std::to_string(n * sizeof(float)) + " bytes could not be allocated: " + e.what());
    }
    launch_rank_live_items(P, rk_items_.p, rk_items_.p + (size_t)mp_.num_item * (size_t)P.pitch, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
    *item_rows = rk_items_.p;
    *item_bias = rk_items_.p + (size_t)mp_.num_item * (size_t)P.pitch;
}

// fb_ptr != nullptr: the sections score with the rows k_rank_live_rows builds from their feedback lists (the configuration has been admitted);
// lines != nullptr: from their USER lines, behind the feedback sum where there is one
void Engine::rank_topn_run(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                           const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out, const RankLines *lines) {
    check(top_n >= 1 && top_n <= RANK_TOPN_MAX,
          "rank_topn: top_n must be between 1 and 256; for longer lists rank the saved model with svdf_ranker_* and top_k");
    // ---- the lists, before any device work
    check(S == 0 || (item_out && count_out && nan_out), "rank_topn: bad arguments");
    RankTopnLists L;
    rank_topn_validate(S, user, ban_ptr, ban_item, (long)mp_.num_user, (long)mp_.num_item, top_n, L);
    if (fb_ptr) rank_fb_validate("rank_topn", S, fb_ptr, fb_index, fb_value, std::min<long>(mp_.num_ufeedback, num_fb_rows()));
    if (lines) rank_lines_admit("rank_topn", S, *lines);
    need_device("rank_topn");
    if (S == 0) return;
    flush();   // behind whatever has been staged
    const float *item_rows = nullptr, *item_bias = nullptr;
    if (lines) rank_live_items("rank_topn", &item_rows, &item_bias);   // once per call
    rank_topn_sweeps("rank_topn", S, user, L, fb_ptr, fb_index, fb_value, lines, item_rows, item_bias, nullptr, top_n, item_out, score_out, count_out, nan_out);
}

// The body the top-N calls share from the upload of the validated lists onward: pieces, geometry, workspace, the launches, the copy-back
// and the count check.  sec_id is the user of each section, or -- query_base != nullptr, svdf_item_topn (svdf_itemtopn.cpp) -- its query
// item, whose row of the [num_item][pitch] matrix query_base is gathered into the piece's row workspace by one more launch.
void Engine::rank_topn_sweeps(const char *who, long S, const unsigned *sec_id, const RankTopnLists &L, const int64_t *fb_ptr, const unsigned *fb_index,
                              const float *fb_value, const RankLines *lines, const float *item_rows, const float *item_bias, const float *query_base,
                              int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    const unsigned *user = sec_id;
    const DevParams &P = params();
    const int N = top_n, cap = rank_topn_cap(P, N);
    const long max_lists = std::max<long>(1, rank_topn_budget_ / cap);
    std::vector<int> in, back;
    for (long s0 = 0; s0 < S;) {
        long s1 = rank_topn_piece(s0, S, max_lists, L.ban_first);
        if (fb_ptr) s1 = rank_fb_piece(who, s0, s1, fb_ptr, rank_eval_budget_);   // ... and at most rank_eval_budget feedback entries
        if (lines) s1 = rank_lines_piece(who, s0, s1, lines->ptr, rank_eval_budget_);   // ... and as many line entries
        const long nsec = s1 - s0;
        const int64_t nban = L.ban_first[(size_t)s1] - L.ban_first[(size_t)s0];
        RankTopnDev D;
        D.nsec = (int)nsec; D.top_n = N; D.cap = cap;
        rank_topn_geometry(P, nsec, max_lists, &D.gy, &D.items_per_block);
        // ---- one upload: sec_user | ban_p0 | ban_item [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        const size_t o_fb = 2 * (size_t)nsec + 1 + (size_t)nban, o_ul = o_fb + (fb_ptr ? rank_fb_words(s0, s1, fb_ptr) : 0);
        in.resize(o_ul + (lines ? rank_lines_words(s0, s1, lines->ptr) : 0));
        if (fb_ptr) rank_fb_pack(s0, s1, fb_ptr, fb_index, fb_value, in.data() + o_fb);
        if (lines) rank_lines_pack(s0, s1, *lines, in.data() + o_ul);
        const size_t o_user = 0, o_bp0 = (size_t)nsec, o_ban = 2 * (size_t)nsec + 1;
        for (long s = s0; s < s1; s++) {
            in[o_user + (size_t)(s - s0)] = (int)user[s];
            in[o_bp0 + (size_t)(s - s0)] = (int)(L.ban_first[(size_t)s] - L.ban_first[(size_t)s0]);
        }
        in[o_bp0 + (size_t)nsec] = (int)nban;
        std::copy(L.ban_ids.begin() + (long)L.ban_first[(size_t)s0], L.ban_ids.begin() + (long)L.ban_first[(size_t)s1], in.begin() + (long)o_ban);
        tn_in_.upload(in.data(), in.size(), stream_);
        // ---- the workspace: list_cnt | nan_cnt | count | items | scores, and the lists
        const size_t nlist = (size_t)nsec * (size_t)D.gy, nres = (size_t)nsec * (2 + 2 * (size_t)N);
        tn_out_.reserve(nlist + nres);
        tn_list_.reserve(nlist * (size_t)cap);
        HIPCHECK(hipMemsetAsync(tn_out_.p, 0, (nlist + (size_t)nsec) * sizeof(int), stream_));
        D.sec_user = reinterpret_cast<const unsigned *>(tn_in_.p + o_user);
        D.ban_p0 = tn_in_.p + o_bp0; D.ban_item = tn_in_.p + o_ban;
        D.user_rows = nullptr;
        D.item_rows = item_rows; D.item_bias = item_bias;
        if (fb_ptr || lines) {   // the sections' effective user rows, one more launch ahead of the sweep
            rk_rows_.reserve((size_t)nsec * (size_t)P.pitch);
            RankLiveRowsDev R;
            R.nsec = (int)nsec; R.sec_user = D.sec_user;
            R.fb_p0 = nullptr; R.fb_index = nullptr; R.fb_value = nullptr;
            if (fb_ptr) {
                const size_t nfb = (size_t)(fb_ptr[s1] - fb_ptr[s0]);
                R.fb_p0 = tn_in_.p + o_fb;
                R.fb_index = reinterpret_cast<const unsigned *>(tn_in_.p + o_fb + (size_t)nsec + 1);
                R.fb_value = reinterpret_cast<const float *>(tn_in_.p + o_fb + (size_t)nsec + 1 + nfb);
                n_rank_fb_sections_ += nsec;
            }
            if (lines) {
                const size_t nul = (size_t)(lines->ptr[s1] - lines->ptr[s0]);
                R.ul_p0 = tn_in_.p + o_ul;
                R.ul_index = reinterpret_cast<const unsigned *>(tn_in_.p + o_ul + (size_t)nsec + 1);
                R.ul_value = reinterpret_cast<const float *>(tn_in_.p + o_ul + (size_t)nsec + 1 + nul);
                n_rank_line_sections_ += nsec;
            }
            R.rows = rk_rows_.p;
            launch_rank_live_rows(P, R, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            D.user_rows = rk_rows_.p;
        } else if (query_base) {   // an item call: the sections' query rows, one more launch ahead of the sweep
            rk_rows_.reserve((size_t)nsec * (size_t)P.pitch);
            launch_item_query_rows(P, query_base, D.sec_user, (int)nsec, rk_rows_.p, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            D.user_rows = rk_rows_.p;
        }
        D.list = tn_list_.p;
        D.list_cnt = tn_out_.p; D.nan_cnt = tn_out_.p + nlist; D.count_out = D.nan_cnt + nsec; D.item_out = D.count_out + nsec;
        D.score_out = reinterpret_cast<float *>(D.item_out + (size_t)nsec * N);
        launch_rank_topn(P, D, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_ += 2;
        // the merge has written the lists as the caller gets them (-1 / 0 beyond a section's count, all of a flagged section): they go
        // straight into the caller's arrays
        back.resize(2 * (size_t)nsec);
        HIPCHECK(hipMemcpyAsync(back.data(), D.nan_cnt, 2 * (size_t)nsec * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(item_out + (size_t)s0 * N, D.item_out, (size_t)nsec * N * sizeof(int), hipMemcpyDeviceToHost, stream_));
        if (score_out) HIPCHECK(hipMemcpyAsync(score_out + (size_t)s0 * N, D.score_out, (size_t)nsec * N * sizeof(float), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        const int *b_nan = back.data(), *b_cnt = b_nan + nsec;
        for (long s = s0; s < s1; s++) {
            const size_t q = (size_t)(s - s0);
            const bool bad = b_nan[q] != 0;
            if (b_cnt[q] != (bad ? 0 : L.count[(size_t)s])) fail(std::string(who) + ": internal error: a section's list is not as long as its candidates allow");
            nan_out[s] = bad ? 1 : 0;
            count_out[s] = b_cnt[q];
        }
        (query_base ? n_item_topn_sections_ : n_rank_topn_sections_) += nsec;
        s0 = s1;
    }
}

}  // namespace svdf

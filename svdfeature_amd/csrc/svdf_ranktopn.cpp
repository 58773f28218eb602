// svdf_ranktopn.cpp -- top-N item lists on the live model: the host side of svdf_rank_topn (refusals, the lists
// through svdf_ranktopn_lists.h, pieces, the workspace of the selecting sweep in svdf_k_ranktopn.hip).
#include <svdfeature_amd.h>

#include <cstring>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_ranktopn_lists.h"

namespace svdf {

// what the batch ranking calls on the live model do not cover (svdf_ranker_* does); `who` is the prefix of the messages
void Engine::rank_live_refusals(const char *who) {
    const std::string w(who);
    if (!(!user_group() && mtype_.extend_type == 0))
        fail(w + ": user-group trainers (format_type = 1) and extend_type != 0 are not covered: the score has a feedback part; rank the saved model with svdf_ranker_*");
    if (!(name_feat_user_ == "NULL" && name_feat_item_ == "NULL"))
        fail(w + ": feature_user / feature_item side tables change the score and are not covered; rank the saved model with svdf_ranker_*");
    if (mp_.common_latent_space != 0) fail(w + ": common_latent_space != 0 is not covered; rank the saved model with svdf_ranker_*");
    if (!(gpus_ == 1 && !multi_)) fail(w + ": amd:gpus > 1 is not covered (the model is spread over the ranks); rank the saved model with svdf_ranker_*");
    if (!(!is_peer_ && !ipc_ && !rccl_))
        fail(w + ": a rank handle of the one-process-per-GPU exchange holds a partition in flight; rank the saved model with svdf_ranker_*");
    if (!(space_allocated_ && trainer_ready_)) fail(w + ": call init_model / load_model and init_trainer first");
}

void Engine::rank_topn(long S, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out,
                       int *count_out, int *nan_out) {
    rank_live_refusals("rank_topn");
    check(top_n >= 1 && top_n <= RANK_TOPN_MAX,
          "rank_topn: top_n must be between 1 and 256; for longer lists rank the saved model with svdf_ranker_* and top_k");
    // ---- the lists, before any device work
    check(S == 0 || (item_out && count_out && nan_out), "rank_topn: bad arguments");
    RankTopnLists L;
    rank_topn_validate(S, user, ban_ptr, ban_item, (long)mp_.num_user, (long)mp_.num_item, top_n, L);
    need_device("rank_topn");
    if (S == 0) return;
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    const int N = top_n, cap = rank_topn_cap(P, N);
    const long max_lists = std::max<long>(1, rank_topn_budget_ / cap);
    std::vector<int> in, back;
    for (long s0 = 0; s0 < S;) {
        const long s1 = rank_topn_piece(s0, S, max_lists, L.ban_first);
        const long nsec = s1 - s0;
        const int64_t nban = L.ban_first[(size_t)s1] - L.ban_first[(size_t)s0];
        RankTopnDev D;
        D.nsec = (int)nsec; D.top_n = N; D.cap = cap;
        rank_topn_geometry(P, nsec, max_lists, &D.gy, &D.items_per_block);
        // ---- one upload: sec_user | ban_p0 | ban_item
        in.resize((size_t)nsec + (size_t)nsec + 1 + (size_t)nban);
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
            check(b_cnt[q] == (bad ? 0 : L.count[(size_t)s]), "rank_topn: internal error: a section's list is not as long as its candidates allow");
            nan_out[s] = bad ? 1 : 0;
            count_out[s] = b_cnt[q];
        }
        n_rank_topn_sections_ += nsec;
        s0 = s1;
    }
}

}  // namespace svdf

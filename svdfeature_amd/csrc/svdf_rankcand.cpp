// svdf_rankcand.cpp -- ranking over per-section candidate lists on the live model: the host side of
// svdf_rank_eval_positions_cand / svdf_rank_topn_cand (refusals, the lists through svdf_rankcand_lists.h, pieces, the one upload and the
// workspaces of the kernels in svdf_k_rankcand.hip).  The sections' rows and the item side come from the paths of sections 6w - 6z.
#include <svdfeature_amd.h>

#include <climits>
#include <cstring>
#include <thread>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankcand_lists.h"
#include "svdf_rankfb_lists.h"
#include "svdf_ranklines_lists.h"

namespace svdf {

template <typename T>
static void rank_cand_reserve(const char *who, DevBuf<T> &buf, size_t n, const char *what) {
    try {
        buf.reserve(n);
    } catch (const std::exception &e) {
        fail(std::string(who) + ": " + what + " of " + std::to_string(n * sizeof(T)) + " bytes could not be allocated: " + e.what());
    }
}

void Engine::rank_cand(const char *who, long S, const unsigned *user, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index,
                       const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *cand_ptr, const unsigned *cand_item, int top_n,
                       int *position_out, int *tied_out, int *ranked_out, int *item_out, float *score_out, int *count_out, int *nan_out) {
    const std::string w(who);
    const bool topn = !strcmp(who, "rank_topn");
    if ((user != nullptr) == (U.ptr != nullptr)) fail(w + ": give the sections either as users or as USER lines");
    const RankLines *lines = U.ptr ? &U : nullptr;
    // what the twin refuses: with users the _fb call's configurations (a format_type = 0 trainer without lists: the plain call's), with
    // USER lines the _lines call's
    if (!rank_live_fb_refusals(who, fb_ptr != nullptr, lines != nullptr)) fb_ptr = nullptr;
    // ---- the lists, before any device work
    if (topn) {
        check(top_n >= 1 && top_n <= RANK_TOPN_MAX,
              "rank_topn: top_n must be between 1 and 256; for longer lists rank the saved model with svdf_ranker_* and top_k");
        check(S >= 0 && (S == 0 || (item_out && count_out && nan_out)), "rank_topn: bad arguments");
        pos_ptr = nullptr;
    } else {
        check(S >= 0 && (S == 0 || (pos_ptr && position_out && tied_out && ranked_out && nan_out)), "rank_eval: bad arguments");
        if (S > 0) {
            check(pos_ptr[0] >= 0, "rank_eval: pos_ptr must start at >= 0");
            for (long s = 0; s < S; s++) check(pos_ptr[s + 1] >= pos_ptr[s], "rank_eval: pos_ptr must not decrease");
            check(pos_ptr[S] == 0 || pos_item, "rank_eval: pos_item is missing");
        }
    }
    rank_cand_validate(who, S, cand_ptr, cand_item, (long)mp_.num_item);
    if (user)
        for (long s = 0; s < S; s++) check(user[s] < (unsigned)mp_.num_user, "user feature index exceed bound");
    RankCandLists L;
    // long calls build their sets on several host threads (sort + unique is the call's largest host part: profiles/r31_rank_cand.md)
    const int64_t entries = S > 0 ? cand_ptr[S] - cand_ptr[0] : 0;
    const int threads = entries < (1 << 18) ? 1 : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    rank_cand_build(S, cand_ptr, cand_item, pos_ptr, pos_item, (long)mp_.num_item, L, threads);
    if (fb_ptr) rank_fb_validate(who, S, fb_ptr, fb_index, fb_value, std::min<long>(mp_.num_ufeedback, num_fb_rows()));
    if (lines) rank_lines_admit(who, S, *lines);
    for (long s = 0; s < S; s++) {
        nan_out[s] = 0;
        if (topn) count_out[s] = 0;
        else ranked_out[s] = L.ranked[(size_t)s];
    }
    need_device(who);
    if (S == 0 || (!topn && pos_ptr[S] == pos_ptr[0])) return;
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    const float *item_rows = nullptr, *item_bias = nullptr;
    if (lines) rank_live_items(who, &item_rows, &item_bias);   // once per call: the whole catalogue, whatever the lists name
    const int N = top_n;
    const int64_t *extra[3] = {pos_ptr, fb_ptr, lines ? lines->ptr : nullptr};
    std::vector<int> in, back, tile_q0, tile_sec;
    for (long s0 = 0; s0 < S;) {
        // ---- a piece of whole sections within the entry budget
        const long s1 = rank_cand_piece(who, s0, S, L.first, extra, 3, rank_eval_budget_);
        const long nsec = s1 - s0;
        const int64_t npair = L.first[(size_t)s1] - L.first[(size_t)s0], npos = topn ? 0 : pos_ptr[s1] - pos_ptr[s0];
        check(npos < INT_MAX / 4 && (!fb_ptr || fb_ptr[s1] - fb_ptr[s0] < INT_MAX / 4) && (!lines || lines->ptr[s1] - lines->ptr[s0] < INT_MAX / 4),
              (w + ": one section with more than 2^29 entries").c_str());
        if (!topn && npos == 0) { s0 = s1; continue; }
        rank_cand_tiles(s0, s1, L.first, tile_q0, tile_sec);
        const int ntile = (int)tile_sec.size();
        // ---- one upload: sec_user | sec_q0 | cand_id | tile_q0 | tile_sec [| sec_p0 | pos_at] [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        in.clear();
        in.reserve(2 * (size_t)nsec + 1 + (size_t)npair + 2 * (size_t)ntile + 1 + (topn ? 0 : (size_t)nsec + 1 + (size_t)npos) +
                   (fb_ptr ? rank_fb_words(s0, s1, fb_ptr) : 0) + (lines ? rank_lines_words(s0, s1, lines->ptr) : 0));
        auto put = [&in](size_t n) { const size_t at = in.size(); in.resize(at + n); return at; };
        const size_t o_user = put((size_t)nsec), o_q0 = put((size_t)nsec + 1), o_id = put((size_t)npair);
        for (long s = s0; s <= s1; s++) {
            if (s < s1) in[o_user + (size_t)(s - s0)] = user ? (int)user[s] : 0;   // (with lines the rows do not read it)
            in[o_q0 + (size_t)(s - s0)] = (int)(L.first[(size_t)s] - L.first[(size_t)s0]);
        }
        std::copy(L.ids.begin() + (long)L.first[(size_t)s0], L.ids.begin() + (long)L.first[(size_t)s1], in.begin() + (long)o_id);
        const size_t o_tq0 = put((size_t)ntile + 1), o_tsec = put((size_t)ntile);
        std::copy(tile_q0.begin(), tile_q0.end(), in.begin() + (long)o_tq0);
        std::copy(tile_sec.begin(), tile_sec.end(), in.begin() + (long)o_tsec);
        size_t o_p0 = 0, o_at = 0;
        if (!topn) {
            o_p0 = put((size_t)nsec + 1);
            o_at = put((size_t)npos);
            for (long s = s0; s <= s1; s++) in[o_p0 + (size_t)(s - s0)] = (int)(pos_ptr[s] - pos_ptr[s0]);
            for (int64_t j = pos_ptr[s0]; j < pos_ptr[s1]; j++)
                in[o_at + (size_t)(j - pos_ptr[s0])] = (int)(L.pos_at[(size_t)(j - pos_ptr[0])] - L.first[(size_t)s0]);
        }
        const size_t o_fb = fb_ptr ? put(rank_fb_words(s0, s1, fb_ptr)) : 0;
        if (fb_ptr) rank_fb_pack(s0, s1, fb_ptr, fb_index, fb_value, in.data() + o_fb);
        const size_t o_ul = lines ? put(rank_lines_words(s0, s1, lines->ptr)) : 0;
        if (lines) rank_lines_pack(s0, s1, *lines, in.data() + o_ul);
        rank_cand_reserve(who, ca_in_, in.size(), "the lists of a piece");
        ca_in_.upload(in.data(), in.size(), stream_);
        // ---- the workspaces: the pairs' scores; position | tied | nan, or nan | count | items | scores
        const size_t nres = topn ? (size_t)nsec * (2 + 2 * (size_t)N) : 2 * (size_t)npos + (size_t)nsec;
        rank_cand_reserve(who, ca_score_, (size_t)npair, "the candidate scores of a piece");
        rank_cand_reserve(who, ca_out_, nres, "the results of a piece");
        RankCandDev D;
        D.nsec = (int)nsec;
        D.sec_user = reinterpret_cast<const unsigned *>(ca_in_.p + o_user);
        D.user_rows = nullptr;
        D.item_rows = item_rows; D.item_bias = item_bias;
        if (fb_ptr || lines) {   // the sections' effective user rows, one more launch ahead of the scores
            rank_cand_reserve(who, rk_rows_, (size_t)nsec * (size_t)P.pitch, "the user rows of a piece");
            RankLiveRowsDev R;
            R.nsec = (int)nsec; R.sec_user = D.sec_user;
            R.fb_p0 = nullptr; R.fb_index = nullptr; R.fb_value = nullptr;
            if (fb_ptr) {
                const size_t nfb = (size_t)(fb_ptr[s1] - fb_ptr[s0]);
                R.fb_p0 = ca_in_.p + o_fb;
                R.fb_index = reinterpret_cast<const unsigned *>(ca_in_.p + o_fb + (size_t)nsec + 1);
                R.fb_value = reinterpret_cast<const float *>(ca_in_.p + o_fb + (size_t)nsec + 1 + nfb);
            }
            if (lines) {
                const size_t nul = (size_t)(lines->ptr[s1] - lines->ptr[s0]);
                R.ul_p0 = ca_in_.p + o_ul;
                R.ul_index = reinterpret_cast<const unsigned *>(ca_in_.p + o_ul + (size_t)nsec + 1);
                R.ul_value = reinterpret_cast<const float *>(ca_in_.p + o_ul + (size_t)nsec + 1 + nul);
            }
            R.rows = rk_rows_.p;
            launch_rank_live_rows(P, R, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            D.user_rows = rk_rows_.p;
        }
        D.sec_q0 = ca_in_.p + o_q0;
        D.cand_id = ca_in_.p + o_id;
        D.cand_score = ca_score_.p;
        D.ntile = ntile;
        D.tile_q0 = ca_in_.p + o_tq0; D.tile_sec = ca_in_.p + o_tsec;
        D.top_n = N;
        if (topn) {
            D.nan_out = ca_out_.p; D.count_out = D.nan_out + nsec; D.item_out = D.count_out + nsec;
            D.score_out = reinterpret_cast<float *>(D.item_out + (size_t)nsec * N);
        } else {
            D.npos = (long)npos;
            D.sec_p0 = ca_in_.p + o_p0; D.pos_at = ca_in_.p + o_at;
            D.position_out = ca_out_.p; D.tied_out = ca_out_.p + npos; D.nan_out = ca_out_.p + 2 * npos;
        }
        launch_rank_cand(P, D, (int)rank_cand_form_, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_ += 1 + (ntile > 0 ? 1 : 0);
        if (topn) {
            // the selection has written the lists as the caller gets them (-1 / 0 beyond a section's count): they go straight into the caller's arrays
            back.resize(2 * (size_t)nsec);
            HIPCHECK(hipMemcpyAsync(back.data(), D.nan_out, 2 * (size_t)nsec * sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIPCHECK(hipMemcpyAsync(item_out + (size_t)s0 * N, D.item_out, (size_t)nsec * N * sizeof(int), hipMemcpyDeviceToHost, stream_));
            if (score_out) HIPCHECK(hipMemcpyAsync(score_out + (size_t)s0 * N, D.score_out, (size_t)nsec * N * sizeof(float), hipMemcpyDeviceToHost, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
            const int *b_nan = back.data(), *b_cnt = b_nan + nsec;
            for (long s = s0; s < s1; s++) {
                const size_t q = (size_t)(s - s0);
                const bool bad = b_nan[q] != 0;
                check(b_cnt[q] == (bad ? 0 : std::min(N, L.ranked[(size_t)s])), "rank_topn: internal error: a section's list is not as long as its candidates allow");
                nan_out[s] = bad ? 1 : 0;
                count_out[s] = b_cnt[q];
            }
            n_rank_topn_sections_ += nsec;
            n_rank_cand_sections_ += nsec;
            if (fb_ptr) n_rank_fb_sections_ += nsec;
            if (lines) n_rank_line_sections_ += nsec;
        } else {
            back.resize(nres);
            HIPCHECK(hipMemcpyAsync(back.data(), ca_out_.p, nres * sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
            for (long s = s0; s < s1; s++) {
                if (pos_ptr[s + 1] == pos_ptr[s]) continue;
                nan_out[s] = back[2 * (size_t)npos + (size_t)(s - s0)] != 0 ? 1 : 0;
                for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {
                    const size_t q = (size_t)(j - pos_ptr[s0]);
                    position_out[j] = back[q];
                    tied_out[j] = back[(size_t)npos + q];
                }
                n_rank_eval_sections_++;
                n_rank_cand_sections_++;
                if (fb_ptr) n_rank_fb_sections_++;
                if (lines) n_rank_line_sections_++;
            }
        }
        s0 = s1;
    }
}

}  // namespace svdf

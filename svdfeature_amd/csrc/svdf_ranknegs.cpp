// svdf_ranknegs.cpp -- live-model ranking against negatives drawn on the device: the host side of
// svdf_rank_eval_positions_sampled (refusals, the excluded lists and the sizes through svdf_ranknegs_lists.h, pieces, the one upload, the
// draw kernel of svdf_k_ranknegs.hip ahead of the score and count kernels of svdf_k_rankcand.hip).  The candidate ids never exist on the
// host: a section's pairs are its positives and num_neg negatives, so the pair offsets and the tile table follow from sizes alone.
#include <svdfeature_amd.h>

#include <climits>
#include <thread>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankcand_lists.h"
#include "svdf_rankfb_lists.h"
#include "svdf_ranklines_lists.h"
#include "svdf_ranknegs_lists.h"

namespace svdf {

template <typename T>
static void rank_negs_reserve(DevBuf<T> &buf, size_t n, const char *what) {
    try {
        buf.reserve(n);
    } catch (const std::exception &e) {
        fail(std::string("rank_eval: ") + what + " of " + std::to_string(n * sizeof(T)) + " bytes could not be allocated: " + e.what());
    }
}

void Engine::rank_negs(long S, const unsigned *user, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                       const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg, uint64_t seed,
                       int *position_out, int *tied_out, int *ranked_out, int *nan_out, int *neg_out) {
    const char *who = "rank_eval";
    if ((user != nullptr) == (U.ptr != nullptr)) fail("rank_eval: give the sections either as users or as USER lines");
    const RankLines *lines = U.ptr ? &U : nullptr;
    if (!rank_live_fb_refusals(who, fb_ptr != nullptr, lines != nullptr)) fb_ptr = nullptr;   // the twins' refusals, in their words
    // ---- the lists, before any device work
    check(S >= 0 && (S == 0 || (pos_ptr && position_out && tied_out && ranked_out && nan_out)), "rank_eval: bad arguments");
    RankNegsLists L;
    // long calls validate and sort their lists on several host threads: this pass is the call's largest host part (profiles/r32_rank_negs.md)
    const int64_t entries = S > 0 && pos_ptr && ban_ptr && pos_ptr[S] >= pos_ptr[0] && ban_ptr[S] >= ban_ptr[0] ? pos_ptr[S] - pos_ptr[0] + ban_ptr[S] - ban_ptr[0] : 0;
    const int threads = entries < (1 << 18) ? 1 : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    rank_negs_build(S, pos_ptr, pos_item, ban_ptr, ban_item, (long)mp_.num_item, num_neg, L, threads);
    if (user)
        for (long s = 0; s < S; s++) check(user[s] < (unsigned)mp_.num_user, "user feature index exceed bound");
    if (fb_ptr) rank_fb_validate(who, S, fb_ptr, fb_index, fb_value, std::min<long>(mp_.num_ufeedback, num_fb_rows()));
    if (lines) rank_lines_admit(who, S, *lines);
    for (long s = 0; s < S; s++) {
        nan_out[s] = 0;
        ranked_out[s] = L.ranked[(size_t)s];
    }
    need_device(who);
    if (S == 0 || pos_ptr[S] == pos_ptr[0]) {
        if (neg_out) std::fill(neg_out, neg_out + (size_t)S * (size_t)num_neg, -1);
        return;
    }
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    const float *item_rows = nullptr, *item_bias = nullptr;
    if (lines) rank_live_items(who, &item_rows, &item_bias);   // once per call
    const int slots = rank_negs_table(num_neg);
    int shift = 32;
    for (int n = slots; n > 1; n >>= 1) shift--;
    const int64_t *extra[4] = {pos_ptr, L.ex_first.data(), fb_ptr, lines ? lines->ptr : nullptr};
    std::vector<int> in, back, tile_q0, tile_sec;
    for (long s0 = 0; s0 < S;) {
        // ---- a piece of whole sections within the entry budget: pairs, positives, excluded ids, feedback and line entries, one per section
        const long s1 = rank_cand_piece(who, s0, S, L.first, extra, 4, rank_eval_budget_);
        const long nsec = s1 - s0;
        const int64_t npair = L.first[(size_t)s1] - L.first[(size_t)s0], npos = pos_ptr[s1] - pos_ptr[s0];
        const int64_t nex = L.ex_first[(size_t)s1] - L.ex_first[(size_t)s0];
        check(npos < INT_MAX / 4 && nex < INT_MAX / 4 && (!fb_ptr || fb_ptr[s1] - fb_ptr[s0] < INT_MAX / 4) &&
                  (!lines || lines->ptr[s1] - lines->ptr[s0] < INT_MAX / 4), "rank_eval: one section with more than 2^29 entries");
        if (npos == 0) {
            if (neg_out) std::fill(neg_out + (size_t)s0 * (size_t)num_neg, neg_out + (size_t)s1 * (size_t)num_neg, -1);
            s0 = s1;
            continue;
        }
        rank_cand_tiles(s0, s1, L.first, tile_q0, tile_sec);
        const int ntile = (int)tile_sec.size();
        // ---- one upload: sec_user | sec_q0 | tile_q0 | tile_sec | sec_p0 | pos_at | pos_id | ex_p0 | ex_id [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        in.clear();
        in.reserve(4 * ((size_t)nsec + 1) + 2 * (size_t)ntile + 1 + 2 * (size_t)npos + (size_t)nex + (fb_ptr ? rank_fb_words(s0, s1, fb_ptr) : 0) +
                   (lines ? rank_lines_words(s0, s1, lines->ptr) : 0));
        auto put = [&in](size_t n) { const size_t at = in.size(); in.resize(at + n); return at; };
        const size_t o_user = put((size_t)nsec), o_q0 = put((size_t)nsec + 1), o_tq0 = put((size_t)ntile + 1), o_tsec = put((size_t)ntile);
        const size_t o_p0 = put((size_t)nsec + 1), o_at = put((size_t)npos), o_pid = put((size_t)npos), o_e0 = put((size_t)nsec + 1), o_ex = put((size_t)nex);
        std::copy(tile_q0.begin(), tile_q0.end(), in.begin() + (long)o_tq0);
        std::copy(tile_sec.begin(), tile_sec.end(), in.begin() + (long)o_tsec);
        for (long s = s0; s <= s1; s++) {
            const size_t q = (size_t)(s - s0);
            if (s < s1) in[o_user + q] = user ? (int)user[s] : 0;   // (with lines the rows do not read it)
            in[o_q0 + q] = (int)(L.first[(size_t)s] - L.first[(size_t)s0]);
            in[o_p0 + q] = (int)(pos_ptr[s] - pos_ptr[s0]);
            in[o_e0 + q] = (int)(L.ex_first[(size_t)s] - L.ex_first[(size_t)s0]);
            if (s < s1)
                for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {   // the positives lead their section's pairs
                    in[o_at + (size_t)(j - pos_ptr[s0])] = in[o_q0 + q] + (int)(j - pos_ptr[s]);
                    in[o_pid + (size_t)(j - pos_ptr[s0])] = (int)pos_item[j];
                }
        }
        std::copy(L.ex_ids.begin() + (long)L.ex_first[(size_t)s0], L.ex_ids.begin() + (long)L.ex_first[(size_t)s1], in.begin() + (long)o_ex);
        const size_t o_fb = fb_ptr ? put(rank_fb_words(s0, s1, fb_ptr)) : 0;
        if (fb_ptr) rank_fb_pack(s0, s1, fb_ptr, fb_index, fb_value, in.data() + o_fb);
        const size_t o_ul = lines ? put(rank_lines_words(s0, s1, lines->ptr)) : 0;
        if (lines) rank_lines_pack(s0, s1, *lines, in.data() + o_ul);
        rank_negs_reserve(ca_in_, in.size(), "the lists of a piece");
        ca_in_.upload(in.data(), in.size(), stream_);
        // ---- the workspaces: the pairs' ids and scores, position | tied | nan, the negatives where they are asked for
        const size_t nres = 2 * (size_t)npos + (size_t)nsec;
        rank_negs_reserve(ng_id_, (size_t)npair, "the candidate ids of a piece");
        rank_negs_reserve(ca_score_, (size_t)npair, "the candidate scores of a piece");
        rank_negs_reserve(ca_out_, nres, "the results of a piece");
        if (neg_out) rank_negs_reserve(ng_neg_, (size_t)nsec * (size_t)num_neg, "the negatives of a piece");
        RankCandDev D;
        D.nsec = (int)nsec;
        D.sec_user = reinterpret_cast<const unsigned *>(ca_in_.p + o_user);
        D.user_rows = nullptr;
        D.item_rows = item_rows; D.item_bias = item_bias;
        if (fb_ptr || lines) {   // the sections' effective user rows, as rank_cand builds them
            rank_negs_reserve(rk_rows_, (size_t)nsec * (size_t)P.pitch, "the user rows of a piece");
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
        RankNegsDev G;
        G.nsec = (int)nsec;
        G.sec0 = s0;
        G.seed = seed;
        G.num_item = (unsigned)mp_.num_item;
        G.num_neg = num_neg;
        G.slots = slots; G.shift = shift;
        G.sec_q0 = ca_in_.p + o_q0;
        G.sec_p0 = ca_in_.p + o_p0; G.pos_id = ca_in_.p + o_pid;
        G.ex_p0 = ca_in_.p + o_e0; G.ex_id = ca_in_.p + o_ex;
        G.cand_id = ng_id_.p;
        G.neg_out = neg_out ? ng_neg_.p : nullptr;
        launch_rank_negs(G, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_++;
        D.sec_q0 = G.sec_q0;
        D.cand_id = ng_id_.p;
        D.cand_score = ca_score_.p;
        D.ntile = ntile;
        D.tile_q0 = ca_in_.p + o_tq0; D.tile_sec = ca_in_.p + o_tsec;
        D.top_n = 0;
        D.npos = (long)npos;
        D.sec_p0 = G.sec_p0; D.pos_at = ca_in_.p + o_at;
        D.position_out = ca_out_.p; D.tied_out = ca_out_.p + npos; D.nan_out = ca_out_.p + 2 * npos;
        launch_rank_cand(P, D, (int)rank_cand_form_, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_ += 1 + (ntile > 0 ? 1 : 0);
        back.resize(nres);
        HIPCHECK(hipMemcpyAsync(back.data(), ca_out_.p, nres * sizeof(int), hipMemcpyDeviceToHost, stream_));
        // the draw kernel has written the rows as the caller gets them (-1 for a section without positives): straight into the caller's array
        if (neg_out)
            HIPCHECK(hipMemcpyAsync(neg_out + (size_t)s0 * (size_t)num_neg, ng_neg_.p, (size_t)nsec * (size_t)num_neg * sizeof(int), hipMemcpyDeviceToHost, stream_));
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
            n_rank_negs_sections_++;
            if (fb_ptr) n_rank_fb_sections_++;
            if (lines) n_rank_line_sections_++;
        }
        s0 = s1;
    }
}

}  // namespace svdf

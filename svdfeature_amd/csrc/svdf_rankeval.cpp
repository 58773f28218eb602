// svdf_rankeval.cpp -- batch ranking evaluation on the live model: the host side of svdf_rank_eval_positions
// (validation, pieces, rows and tiles of the sweep in svdf_k_rankeval.hip) and the reference's ranking metrics over positions
// (apex-utils/apex_evaluator.h:33-215), which need no GPU.
#include <svdfeature_amd.h>

#include <climits>
#include <cstring>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankeval_lists.h"
#include "svdf_rankfb_lists.h"
#include "svdf_ranklines_lists.h"
#include "svdf_ranktopn_lists.h"

namespace svdf {

// EvaluatorMAP::add_eval(pos_idx, false) per section and the sums print_result divides by ninst.  `sum_ar` is the reference's
// std::vector<float>: the running sum MAP@k reads has been rounded to float, and `sum_ar[j - 1] / pos_idx.size()` is a FLOAT division
// (the size converts to float) whose quotient is then added in double.
void rank_eval_metrics(long S, const int64_t *sec_ptr, const int *position, const int *ranked, const int *nan, int num_at, const int *at,
                       svdf_rank_metrics *out) {
    check(S >= 0 && (S == 0 || sec_ptr) && out, "rank_eval_metrics: bad arguments");
    check(num_at >= 0 && num_at <= 8 && (num_at == 0 || at), "rank_eval_metrics: up to 8 cut-offs");
    memset(out, 0, sizeof(*out));
    out->num_at = num_at;
    for (int i = 0; i < num_at; i++) { check(at[i] >= 1, "rank_eval_metrics: a cut-off must be at least 1"); out->at[i] = at[i]; }
    std::sort(out->at, out->at + num_at);   // init(): the at lists are sorted
    if (S > 0) check(sec_ptr[0] >= 0, "rank_eval_metrics: section pointers must start at >= 0");
    std::vector<int> pos;
    std::vector<float> sum_ar;
    for (long s = 0; s < S; s++) {
        check(sec_ptr[s + 1] >= sec_ptr[s], "rank_eval_metrics: section pointers must not decrease");
        const size_t n = (size_t)(sec_ptr[s + 1] - sec_ptr[s]);
        if (n == 0) { out->skipped++; continue; }   // add_eval would assert: "no positive record presented"
        if (nan && nan[s]) { out->nan_sections++; continue; }
        pos.assign(position + sec_ptr[s], position + sec_ptr[s + 1]);
        std::sort(pos.begin(), pos.end());
        check(pos[0] >= 0, "rank_eval_metrics: negative position in a section that is not flagged");
        double sumap = 0.0;
        sum_ar.clear();
        for (size_t i = 0; i < n; i++) {
            const double pp = ((double)(i + 1)) / (pos[i] + 1);
            sumap += pp;
            sum_ar.push_back((float)sumap);
        }
        out->sum_map += sumap / n;
        size_t j = 0;
        for (int i = 0; i < num_at; i++) {
            while (j < n && pos[j] < out->at[i]) j++;
            if (j != 0) out->sum_map_at[i] += sum_ar[j - 1] / n;
        }
        j = 0;
        for (int i = 0; i < num_at; i++) {
            while (j < n && pos[j] < out->at[i]) j++;
            out->sum_pre_at[i] += ((double)j) / out->at[i];
        }
        j = 0;
        for (int i = 0; i < num_at; i++) {
            while (j < n && pos[j] < out->at[i]) j++;
            out->sum_rec_at[i] += ((double)j) / n;
        }
        out->ninst++;
        if (ranked && (int64_t)ranked[s] > (int64_t)n) {   // AUC (not in the reference): the share of (positive, other ranked candidate) pairs in the right order
            int64_t above = 0;
            for (size_t i = 0; i < n; i++) above += (int64_t)pos[i] - (int64_t)i;
            out->sum_auc += 1.0 - (double)above / ((double)n * (double)((int64_t)ranked[s] - (int64_t)n));
            out->nauc++;
        }
    }
}

void Engine::rank_eval_positions(long S, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                                 const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out) {
    rank_live_refusals("rank_eval");   // what the batch call does not cover (svdf_ranker_* does): svdf_ranktopn.cpp
    rank_eval_run(S, user, nullptr, nullptr, nullptr, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
}

// the same on a user-group trainer, whose sections bring feedback lists; without lists on a format_type = 0 trainer: the call above
void Engine::rank_eval_positions_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                    const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out,
                                    int *tied_out, int *ranked_out, int *nan_out) {
    if (!rank_live_fb_refusals("rank_eval", fb_ptr != nullptr)) fb_ptr = nullptr;
    rank_eval_run(S, user, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
}

// ... and for sections that bring a USER line, on trainers with or without side tables
void Engine::rank_eval_positions_lines(long S, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                       const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                                       int *position_out, int *tied_out, int *ranked_out, int *nan_out) {
    if (!rank_live_fb_refusals("rank_eval", fb_ptr != nullptr, true)) fb_ptr = nullptr;
    const std::vector<unsigned> user((size_t)std::max<long>(S, 1), 0u);   // not read by the kernels: the rows come from the lines
    rank_eval_run(S, user.data(), fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out, &U);
}

// fb_ptr != nullptr: the sections score with the rows k_rank_live_rows builds from their feedback lists (the configuration has been admitted);
// lines != nullptr: from their USER lines, behind the feedback sum where there is one
void Engine::rank_eval_run(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                           const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out,
                           int *nan_out, const RankLines *lines) {
    // ---- the lists, before any device work
    check(S >= 0 && (S == 0 || (user && pos_ptr)), "rank_eval: bad arguments");
    const long num_item = mp_.num_item;
    std::vector<int64_t> ban_first((size_t)S + 1, 0);   // distinct (section, banned id) pairs of sections WITH positives: [ban_first[s], ban_first[s + 1])
    std::vector<int> ban_ids;
    if (S > 0) {
        check(pos_ptr[0] >= 0, "rank_eval: pos_ptr must start at >= 0");
        check(!ban_ptr || ban_ptr[0] >= 0, "rank_eval: ban_ptr must start at >= 0");
        for (long s = 0; s < S; s++) {
            check(pos_ptr[s + 1] >= pos_ptr[s], "rank_eval: pos_ptr must not decrease");
            check(!ban_ptr || ban_ptr[s + 1] >= ban_ptr[s], "rank_eval: ban_ptr must not decrease");
        }
        check(pos_ptr[S] == 0 || pos_item, "rank_eval: pos_item is missing");
        check(!ban_ptr || ban_ptr[S] == 0 || ban_item, "rank_eval: ban_item is missing");
        std::vector<long> stamp((size_t)num_item, 0);   // 2 s + 1: banned in section s, 2 s + 2: positive of section s
        for (long s = 0; s < S; s++) {
            check(user[s] < (unsigned)mp_.num_user, "user feature index exceed bound");
            long nban = 0;
            const bool keep = pos_ptr[s + 1] > pos_ptr[s];
            if (ban_ptr)
                for (int64_t j = ban_ptr[s]; j < ban_ptr[s + 1]; j++) {
                    const unsigned b = ban_item[j];
                    check((long)b < num_item, "sample item index exceed bound");
                    if (stamp[b] == 2 * s + 1) continue;   // the ranker's tag write is idempotent
                    stamp[b] = 2 * s + 1;
                    nban++;
                    if (keep) ban_ids.push_back((int)b);
                }
            for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {
                const unsigned p = pos_item[j];
                check((long)p < num_item, "sample item index exceed bound");
                check(stamp[p] != 2 * s + 1, "each pos sample item can not occur in baned sample list");
                check(stamp[p] != 2 * s + 2, "rank_eval: a positive item is repeated inside a section");
                stamp[p] = 2 * s + 2;
            }
            ban_first[(size_t)s + 1] = (int64_t)ban_ids.size();
            ranked_out[s] = (int)(num_item - nban);
            nan_out[s] = 0;
        }
    }
    if (fb_ptr) rank_fb_validate("rank_eval", S, fb_ptr, fb_index, fb_value, std::min<long>(mp_.num_ufeedback, num_fb_rows()));
    if (lines) rank_lines_admit("rank_eval", S, *lines);
    need_device("rank_eval");
    if (S == 0 || pos_ptr[S] == pos_ptr[0]) return;
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    const float *item_rows = nullptr, *item_bias = nullptr;
    if (lines) rank_live_items("rank_eval", &item_rows, &item_bias);   // once per call
    const int tile_rows = rank_eval_tile_rows(P);
    std::vector<int> in, back;
    for (long s0 = 0; s0 < S;) {
        // ---- a piece of whole sections within the device budget
        const long s1 = rank_eval_piece(s0, S, rank_eval_budget_, [&](long s) {
            return (pos_ptr[s + 1] - pos_ptr[s]) + (ban_first[(size_t)s + 1] - ban_first[(size_t)s]) + 1 + (fb_ptr ? fb_ptr[s + 1] - fb_ptr[s] : 0) +
                   (lines ? lines->ptr[s + 1] - lines->ptr[s] : 0);
        });
        const long nsec = s1 - s0;
        const int64_t npos = pos_ptr[s1] - pos_ptr[s0], nban = ban_first[(size_t)s1] - ban_first[(size_t)s0];
        check(npos < INT_MAX / 4 && nban < INT_MAX / 4 && (!fb_ptr || fb_ptr[s1] - fb_ptr[s0] < INT_MAX / 4) &&
                  (!lines || lines->ptr[s1] - lines->ptr[s0] < INT_MAX / 4), "rank_eval: one section with more than 2^29 entries");
        if (npos == 0) { s0 = s1; continue; }
        // ---- rows (a section, or a slice of its positives) and tiles of rows
        RankEvalRows rows;
        rank_eval_rows(pos_ptr, s0, s1, tile_rows, RANK_EVAL_TILE_POS, rows);
        const std::vector<int> &row_sec = rows.row_sec, &row_first = rows.row_first, &row_p0 = rows.row_p0, &tile_r0 = rows.tile_r0;
        const int nrow = rows.nrow(), ntile = rows.ntile();
        // ---- one upload: sec_user | sec_p0 | pos_item | pos_sec | row_sec | row_first | row_p0 | tile_r0 | ban_sec | ban_item [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        in.clear();
        in.reserve(2 * (size_t)nsec + 1 + 2 * (size_t)npos + 3 * (size_t)nrow + 1 + (size_t)ntile + 1 + 2 * (size_t)nban +
                   (fb_ptr ? rank_fb_words(s0, s1, fb_ptr) : 0) + (lines ? rank_lines_words(s0, s1, lines->ptr) : 0));   // one allocation: the parts below never move what is already there
        auto put =[&in](size_t n) { const size_t at = in.size(); in.resize(at + n); return at; };
        const size_t o_user = put((size_t)nsec), o_sp0 = put((size_t)nsec + 1), o_pitem = put((size_t)npos), o_psec = put((size_t)npos);
        for (long s = s0; s < s1; s++) {
            in[o_user + (size_t)(s - s0)] = (int)user[s];
            in[o_sp0 + (size_t)(s - s0)] = (int)(pos_ptr[s] - pos_ptr[s0]);
            for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {
                in[o_pitem + (size_t)(j - pos_ptr[s0])] = (int)pos_item[j];
                in[o_psec + (size_t)(j - pos_ptr[s0])] = (int)(s - s0);
            }
        }
        in[o_sp0 + (size_t)nsec] = (int)npos;
        const size_t o_rsec = put((size_t)nrow), o_rfirst = put((size_t)nrow), o_rp0 = put((size_t)nrow + 1), o_tile = put((size_t)ntile + 1);
        std::copy(row_sec.begin(), row_sec.end(), in.begin() + (long)o_rsec);
        std::copy(row_first.begin(), row_first.end(), in.begin() + (long)o_rfirst);
        std::copy(row_p0.begin(), row_p0.end(), in.begin() + (long)o_rp0);
        std::copy(tile_r0.begin(), tile_r0.end(), in.begin() + (long)o_tile);
        const size_t o_bsec = put((size_t)nban), o_bitem = put((size_t)nban);
        for (long s = s0; s < s1; s++)
            for (int64_t j = ban_first[(size_t)s]; j < ban_first[(size_t)s + 1]; j++) {
                in[o_bsec + (size_t)(j - ban_first[(size_t)s0])] = (int)(s - s0);
                in[o_bitem + (size_t)(j - ban_first[(size_t)s0])] = ban_ids[(size_t)j];
            }
        const size_t o_fb = fb_ptr ? put(rank_fb_words(s0, s1, fb_ptr)) : 0;
        if (fb_ptr) rank_fb_pack(s0, s1, fb_ptr, fb_index, fb_value, in.data() + o_fb);
        const size_t o_ul = lines ? put(rank_lines_words(s0, s1, lines->ptr)) : 0;
        if (lines) rank_lines_pack(s0, s1, *lines, in.data() + o_ul);
        re_in_.upload(in.data(), in.size(), stream_);
        const size_t ncnt = 3 * (size_t)npos + (size_t)nsec;
        re_cnt_.reserve(ncnt);
        re_ps_.reserve((size_t)npos);
        HIPCHECK(hipMemsetAsync(re_cnt_.p, 0, ncnt * sizeof(int), stream_));
        RankEvalDev D;
        D.nsec = (int)nsec;
        D.sec_user = reinterpret_cast<const unsigned *>(re_in_.p + o_user);
        D.user_rows = nullptr;
        D.item_rows = item_rows; D.item_bias = item_bias;
        if (fb_ptr || lines) {   // the sections' effective user rows, one more launch ahead of the sweep
            rk_rows_.reserve((size_t)nsec * (size_t)P.pitch);
            RankLiveRowsDev R;
            R.nsec = (int)nsec; R.sec_user = D.sec_user;
            R.fb_p0 = nullptr; R.fb_index = nullptr; R.fb_value = nullptr;
            if (fb_ptr) {
                const size_t nfb = (size_t)(fb_ptr[s1] - fb_ptr[s0]);
                R.fb_p0 = re_in_.p + o_fb;
                R.fb_index = reinterpret_cast<const unsigned *>(re_in_.p + o_fb + (size_t)nsec + 1);
                R.fb_value = reinterpret_cast<const float *>(re_in_.p + o_fb + (size_t)nsec + 1 + nfb);
            }
            if (lines) {
                const size_t nul = (size_t)(lines->ptr[s1] - lines->ptr[s0]);
                R.ul_p0 = re_in_.p + o_ul;
                R.ul_index = reinterpret_cast<const unsigned *>(re_in_.p + o_ul + (size_t)nsec + 1);
                R.ul_value = reinterpret_cast<const float *>(re_in_.p + o_ul + (size_t)nsec + 1 + nul);
            }
            R.rows = rk_rows_.p;
            launch_rank_live_rows(P, R, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            D.user_rows = rk_rows_.p;
        }
        D.sec_p0 = re_in_.p + o_sp0;
        D.npos = (long)npos;
        D.pos_item = re_in_.p + o_pitem; D.pos_sec = re_in_.p + o_psec;
        D.pos_score = re_ps_.p;
        D.greater = re_cnt_.p; D.tied = re_cnt_.p + npos; D.before = re_cnt_.p + 2 * npos; D.nan_cnt = re_cnt_.p + 3 * npos;
        D.nrow = nrow; D.ntile = ntile;
        D.row_sec = re_in_.p + o_rsec; D.row_first = re_in_.p + o_rfirst; D.row_p0 = re_in_.p + o_rp0; D.tile_r0 = re_in_.p + o_tile;
        D.nban = (long)nban;
        D.ban_sec = re_in_.p + o_bsec; D.ban_item = re_in_.p + o_bitem;
        launch_rank_eval(P, D, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_ += 2 + (nban > 0 ? 1 : 0);
        back.resize(ncnt);
        HIPCHECK(hipMemcpyAsync(back.data(), re_cnt_.p, ncnt * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        for (long s = s0; s < s1; s++) {
            if (pos_ptr[s + 1] == pos_ptr[s]) continue;
            const bool bad = back[3 * (size_t)npos + (size_t)(s - s0)] != 0;
            nan_out[s] = bad ? 1 : 0;
            for (int64_t j = pos_ptr[s]; j < pos_ptr[s + 1]; j++) {
                const size_t q = (size_t)(j - pos_ptr[s0]);
                position_out[j] = bad ? -1 : back[q] + back[2 * (size_t)npos + q];
                tied_out[j] = bad ? -1 : back[(size_t)npos + q];
            }
            n_rank_eval_sections_++;
            if (fb_ptr) n_rank_fb_sections_++;
            if (lines) n_rank_line_sections_++;
        }
        s0 = s1;
    }
}

// The test probe svdf_rank_geometry: what the launches of the two calls would be told, from the functions they call, without a device.
// Only the row width, the item count and the two budgets of the handle matter, so the parameters need not be followed by init_model.
void Engine::rank_geometry(int kind, long units, int top_n, const int64_t *pos_ptr, long *out) {
    check((kind == 0 || kind == 1) && units >= 1 && out, "rank_geometry: bad arguments");
    check(mp_.num_factor >= 1 && mp_.num_item >= 1, "rank_geometry: set num_factor and num_item first");
    DevParams P;
    memset(&P, 0, sizeof(P));
    P.pitch = row_pitch(mp_.num_factor); P.k = mp_.num_factor; P.num_item = mp_.num_item;   // before init_model too
    for (int i = 0; i < 8; i++) out[i] = 0;
    int gy = 0;
    long per = 0;
    if (kind == 0) {
        const int tile_rows = rank_eval_tile_rows(P);
        long ntile = units, nrow = 0, piece = 0;
        if (pos_ptr) {   // units sections without bans, feedback or lines: the first piece, its rows and tiles
            check(pos_ptr[0] >= 0, "rank_geometry: pos_ptr must start at >= 0");
            for (long s = 0; s < units; s++) check(pos_ptr[s + 1] >= pos_ptr[s], "rank_geometry: pos_ptr must not decrease");
            piece = rank_eval_piece(0, units, rank_eval_budget_, [&](long s) { return pos_ptr[s + 1] - pos_ptr[s] + 1; });
            RankEvalRows rows;
            rank_eval_rows(pos_ptr, 0, piece, tile_rows, RANK_EVAL_TILE_POS, rows);
            nrow = rows.nrow(); ntile = rows.ntile();
        }
        if (ntile > 0) rank_eval_geometry(P, ntile, &gy, &per);
        out[3] = tile_rows; out[4] = nrow; out[5] = ntile; out[6] = piece;
        out[7] = P.pitch <= 256 ? (ntile > 0 ? 1 : 0) : (nrow + RANK_EVAL_WIDE_ROWS - 1) / RANK_EVAL_WIDE_ROWS;   // launches of the sweep
    } else {
        check(top_n >= 1 && top_n <= RANK_TOPN_MAX, "rank_geometry: top_n must be between 1 and 256");
        const int cap = rank_topn_cap(P, top_n);
        const long max_lists = std::max<long>(1, rank_topn_budget_ / cap);
        const std::vector<int64_t> no_bans((size_t)units + 1, 0);
        const long piece = rank_topn_piece(0, units, max_lists, no_bans);   // units sections without bans: the first piece
        rank_topn_geometry(P, piece, max_lists, &gy, &per);
        const long ts = rank_topn_tile_rows(P);
        out[2] = cap; out[3] = ts; out[4] = piece; out[5] = (piece + ts - 1) / ts; out[6] = piece; out[7] = 1;
    }
    out[0] = gy; out[1] = per;
}

}  // namespace svdf

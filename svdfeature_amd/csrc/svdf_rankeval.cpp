// svdf_rankeval.cpp -- batch ranking evaluation on the live model: the host side of svdf_rank_eval_positions
// (validation, pieces, rows and tiles of the sweep in svdf_k_rankeval.hip) and the reference's ranking metrics over positions
// (apex-utils/apex_evaluator.h:33-215), which need no GPU.
#include <svdfeature_amd.h>

#include <climits>
#include <cstring>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_rankeval_lists.h"
#include "svdf_rankrows_lists.h"
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
    RankRowSource R;
    R.user = user;
    rank_eval_run(S, R, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
}

// the same on a user-group trainer, whose sections bring feedback lists; without lists on a format_type = 0 trainer: the call above
void Engine::rank_eval_positions_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                    const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out,
                                    int *tied_out, int *ranked_out, int *nan_out) {
    RankRowSource R;
    R.user = user;
    if (rank_live_fb_refusals("rank_eval", fb_ptr != nullptr)) R.fb = RankList{fb_ptr, fb_index, fb_value};
    rank_eval_run(S, R, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
}

// ... and for sections that bring a USER line, on trainers with or without side tables
void Engine::rank_eval_positions_lines(long S, const RankList &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                       const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                                       int *position_out, int *tied_out, int *ranked_out, int *nan_out) {
    RankRowSource R;   // no users: the rows come from the lines
    R.lines = U; R.by_lines = true;
    if (rank_live_fb_refusals("rank_eval", fb_ptr != nullptr, true)) R.fb = RankList{fb_ptr, fb_index, fb_value};
    rank_eval_run(S, R, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
}

// R.fb given: the sections score with the rows k_rank_live_rows builds from their feedback lists (the configuration has been admitted);
// R.lines given: from their USER lines, behind the feedback sum where there is one.
// Under the knob rank_eval_prefilter (prefilter_ok: not the second run below) the pieces go through the counting sweep
// on the matrix cores and the band pass (launch_rank_eval_mx); the sections the rule does not certify are gathered -- users, positives, the
// validated ban lists, feedback lists, USER lines -- into contiguous copies, ranked once more by this function with the route off and
// scattered to their places.  Either way every count is the pinned sweep's.
void Engine::rank_eval_run(long S, RankRowSource R, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                           int *position_out, int *tied_out, int *ranked_out, int *nan_out, bool prefilter_ok) {
    const bool mx = prefilter_ok && rank_eval_prefilter_ != 0;
    // ---- the lists, before any device work
    check(S >= 0 && (S == 0 || ((R.user || R.by_lines) && pos_ptr)), "rank_eval: bad arguments");
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
            check(!R.user || R.user[s] < (unsigned)mp_.num_user, "user feature index exceed bound");
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
            if (mx) std::sort(ban_ids.begin() + (long)ban_first[(size_t)s], ban_ids.end());   // the matrix sweep walks a section's bans by ascending cursors
            ban_first[(size_t)s + 1] = (int64_t)ban_ids.size();
            ranked_out[s] = (int)(num_item - nban);
            nan_out[s] = 0;
        }
    }
    rank_rows_validate("rank_eval", S, R);
    need_device("rank_eval");
    if (S == 0 || pos_ptr[S] == pos_ptr[0]) return;
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    if (R.lines.ptr) rank_live_items("rank_eval", R);   // once per call
    const int tile_rows = mx ? 64 : rank_eval_tile_rows(P), tile_pos = mx ? RANK_EVAL_MX_POS : RANK_EVAL_TILE_POS;
    // under the prefilter a section's band lists count into the piece budget
    auto band_cost = [&](long s) { return mx ? rank_eval_band_cost(pos_ptr[s + 1] - pos_ptr[s], rank_eval_band_, tile_pos) : 0; };
    if (mx) rank_item_envelope("rank_eval", R);
    std::vector<long> again;   // sections the rule did not certify
    std::vector<int> in, back;
    for (long s0 = 0; s0 < S;) {
        // a piece always takes its first section: one whose band lists alone exceed the budget (rows x capacity ids) is ranked by the
        // pinned route, not given a workspace of that size
        if (band_cost(s0) > (int64_t)rank_eval_budget_) {
            rank_sections_counted(R, 1);
            n_rank_eval_again_++;
            again.push_back(s0++);
            continue;
        }
        // ---- a piece of whole sections within the device budget
        const long s1 = rank_eval_piece(s0, S, rank_eval_budget_, [&](long s) {
            return (pos_ptr[s + 1] - pos_ptr[s]) + (ban_first[(size_t)s + 1] - ban_first[(size_t)s]) + 1 + (R.fb.ptr ? R.fb.ptr[s + 1] - R.fb.ptr[s] : 0) +
                   (R.lines.ptr ? R.lines.ptr[s + 1] - R.lines.ptr[s] : 0) + band_cost(s);
        });
        const long nsec = s1 - s0;
        const int64_t npos = pos_ptr[s1] - pos_ptr[s0], nban = ban_first[(size_t)s1] - ban_first[(size_t)s0];
        check(npos < INT_MAX / 4 && nban < INT_MAX / 4 && (!R.fb.ptr || R.fb.ptr[s1] - R.fb.ptr[s0] < INT_MAX / 4) &&
                  (!R.lines.ptr || R.lines.ptr[s1] - R.lines.ptr[s0] < INT_MAX / 4), "rank_eval: one section with more than 2^29 entries");
        if (npos == 0) { s0 = s1; continue; }
        // ---- rows (a section, or a slice of its positives) and tiles of rows
        RankEvalRows rows;
        rank_eval_rows(pos_ptr, s0, s1, tile_rows, tile_pos, rows);
        const std::vector<int> &row_sec = rows.row_sec, &row_first = rows.row_first, &row_p0 = rows.row_p0, &tile_r0 = rows.tile_r0;
        const int nrow = rows.nrow(), ntile = rows.ntile();
        // (under the prefilter ban_p0 [nsec + 1] stands in ban_sec's place and the ids are ascending inside a section)
        // ---- one upload: sec_user | sec_p0 | pos_item | pos_sec | row_sec | row_first | row_p0 | tile_r0 | ban_sec | ban_item [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
        in.clear();
        in.reserve(2 * (size_t)nsec + 1 + 2 * (size_t)npos + 3 * (size_t)nrow + 1 + (size_t)ntile + 1 + 2 * (size_t)nban + (mx ? (size_t)nsec + 1 : 0) +
                   rank_rows_words(R, s0, s1));   // one allocation: the parts below never move what is already there
        auto put =[&in](size_t n) { const size_t at = in.size(); in.resize(at + n); return at; };
        const size_t o_user = put((size_t)nsec), o_sp0 = put((size_t)nsec + 1), o_pitem = put((size_t)npos), o_psec = put((size_t)npos);
        for (long s = s0; s < s1; s++) {
            in[o_user + (size_t)(s - s0)] = R.user_of(s);
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
        const size_t o_bsec = put(mx ? (size_t)nsec + 1 : (size_t)nban), o_bitem = put((size_t)nban);
        for (long s = s0; s < s1; s++) {
            if (mx) in[o_bsec + (size_t)(s - s0)] = (int)(ban_first[(size_t)s] - ban_first[(size_t)s0]);
            for (int64_t j = ban_first[(size_t)s]; j < ban_first[(size_t)s + 1]; j++) {
                if (!mx) in[o_bsec + (size_t)(j - ban_first[(size_t)s0])] = (int)(s - s0);
                in[o_bitem + (size_t)(j - ban_first[(size_t)s0])] = ban_ids[(size_t)j];
            }
        }
        if (mx) in[o_bsec + (size_t)nsec] = (int)nban;
        const RankRowsAt o_rows = rank_rows_pack(R, s0, s1, in);
        reserve_or_fail("rank_eval", re_in_, in.size(), "the lists of a piece");
        re_in_.upload(in.data(), in.size(), stream_);
        // the counts: greater | tied | before [npos] | nan_cnt [nsec]; under the prefilter also sec_ok [nsec] | row_cert [nrow] | band_cursor [nrow]
        const size_t ncnt = 3 * (size_t)npos + (size_t)nsec + (mx ? (size_t)nsec + 2 * (size_t)nrow : 0);
        reserve_or_fail("rank_eval", re_cnt_, ncnt, "the counts of a piece");
        reserve_or_fail("rank_eval", re_ps_, (mx ? 3 : 1) * (size_t)npos, "the positives' scores of a piece");
        if (mx) reserve_or_fail("rank_eval", re_band_, (size_t)npos + (size_t)nrow * (size_t)rank_eval_band_, "the band lists of a piece");
        HIPCHECK(hipMemsetAsync(re_cnt_.p, 0, ncnt * sizeof(int), stream_));
        RankEvalMxDev D;
        D.nsec = (int)nsec;
        D.sec_user = reinterpret_cast<const unsigned *>(re_in_.p + o_user);
        D.item_rows = R.item_rows; D.item_bias = R.item_bias;
        D.user_rows = rank_rows_launch("rank_eval", R, re_in_.p, o_rows, D.sec_user, s0, s1);
        D.sec_p0 = re_in_.p + o_sp0;
        D.npos = (long)npos;
        D.pos_item = re_in_.p + o_pitem; D.pos_sec = re_in_.p + o_psec;
        D.pos_score = re_ps_.p;
        D.greater = re_cnt_.p; D.tied = re_cnt_.p + npos; D.before = re_cnt_.p + 2 * npos; D.nan_cnt = re_cnt_.p + 3 * npos;
        D.nrow = nrow; D.ntile = ntile;
        D.row_sec = re_in_.p + o_rsec; D.row_first = re_in_.p + o_rfirst; D.row_p0 = re_in_.p + o_rp0; D.tile_r0 = re_in_.p + o_tile;
        D.nban = (long)nban;
        D.ban_sec = re_in_.p + o_bsec; D.ban_item = re_in_.p + o_bitem;
        if (mx) {
            D.ban_sec = nullptr; D.ban_p0 = re_in_.p + o_bsec;
            D.envelope = tn_env_.p;
            rank_topn_geometry(P, nrow, LONG_MAX, &D.gy, &D.items_per_block, 1);   // 64-row units, tiles of 128 items, about 2 048 workgroups
            D.srt = re_band_.p; D.band_list = re_band_.p + npos; D.band_cap = rank_eval_band_;
            D.lo = re_ps_.p + npos; D.hi = re_ps_.p + 2 * npos;
            D.sec_ok = D.nan_cnt + nsec; D.row_cert = D.sec_ok + nsec; D.band_cursor = D.row_cert + nrow;
            launch_rank_eval_mx(P, D, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_ += 4;
        } else {
            launch_rank_eval(P, D, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_ += 2 + (nban > 0 ? 1 : 0);
        }
        back.resize(ncnt);
        HIPCHECK(hipMemcpyAsync(back.data(), re_cnt_.p, ncnt * sizeof(int), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        // the position of a positive is greater + before; all of a flagged section: -1
        int *const b_pos = back.data(), *const b_tied = b_pos + npos, *const b_before = b_tied + npos, *const b_nan = b_before + npos;
        for (long s = s0; s < s1; s++)
            for (int64_t q = pos_ptr[s] - pos_ptr[s0]; q < pos_ptr[s + 1] - pos_ptr[s0]; q++) {
                b_pos[q] = b_nan[s - s0] ? -1 : b_pos[q] + b_before[q];
                if (b_nan[s - s0]) b_tied[q] = -1;
            }
        if (!mx) {
            rank_positions_back(R, pos_ptr, s0, s1, b_pos, b_tied, b_nan, position_out, tied_out, nan_out);
            s0 = s1;
            continue;
        }
        const int *const b_ok = b_nan + nsec, *const b_cert = b_ok + nsec, *const b_cursor = b_cert + nrow;
        for (size_t i = 0; i < (size_t)nrow; i++) {
            n_rank_eval_band_rows_++; n_rank_eval_band_ids_ += b_cursor[i];
            n_rank_eval_band_max_ = std::max<int64_t>(n_rank_eval_band_max_, b_cursor[i]);
        }
        size_t r = 0;   // the first row of section s
        for (long s = s0; s < s1; s++) {
            if (pos_ptr[s + 1] == pos_ptr[s]) continue;
            // certified: (a), (b) by k_rank_eval_prep, (c) no NaN in the sweep, (d) and the pinned NaN check by every row's word
            bool cert = !b_nan[s - s0] && b_ok[s - s0] != 0;
            for (; r < (size_t)nrow && row_sec[r] == (int)(s - s0); r++) cert = cert && b_cert[r] != 0;
            if (cert) {
                n_rank_eval_certified_++;
                // section s as a piece of its own: with pos_ptr and nan_out shifted to s, the routine's s0 = 0 reads pos_ptr[s], pos_ptr[s + 1]
                // and writes nan_out[s], and its sources start at the section's first positive and at its nan word (0: certified)
                rank_positions_back(R, pos_ptr + s, 0, 1, b_pos + (pos_ptr[s] - pos_ptr[s0]), b_tied + (pos_ptr[s] - pos_ptr[s0]), b_nan + (s - s0),
                                    position_out, tied_out, nan_out + s);
            } else {
                rank_sections_counted(R, 1);
                n_rank_eval_again_++;
                again.push_back(s);
            }
        }
        s0 = s1;
    }
    if (again.empty()) return;
    // ---- the sections left: contiguous copies of what they bring, this function with the route off, the results back to their places
    const RankRelist X(again, R, ban_first, ban_ids);
    const long A = (long)again.size();
    std::vector<unsigned> a_pos;
    std::vector<int64_t> a_pp((size_t)A + 1, 0);
    for (long a = 0; a < A; a++) {
        a_pos.insert(a_pos.end(), pos_item + pos_ptr[again[(size_t)a]], pos_item + pos_ptr[again[(size_t)a] + 1]);
        a_pp[(size_t)a + 1] = (int64_t)a_pos.size();
    }
    std::vector<int> a_position(a_pos.size()), a_tied(a_pos.size()), a_ranked((size_t)A), a_nan((size_t)A);
    const int64_t c38 = n_rank_eval_sections_, c40 = n_rank_fb_sections_, c41 = n_rank_line_sections_;   // each section counts once
    rank_eval_run(A, X.rows, a_pp.data(), a_pos.data(), X.ban_first.data(), reinterpret_cast<const unsigned *>(X.ban_ids.data()), a_position.data(),
                  a_tied.data(), a_ranked.data(), a_nan.data(), false);
    n_rank_eval_sections_ = c38; n_rank_fb_sections_ = c40; n_rank_line_sections_ = c41;
    auto one = [](long i) { return i; };
    X.scatter(a_position.data(), [&](long a) { return a_pp[(size_t)a]; }, position_out, [&](long s) { return pos_ptr[s]; });
    X.scatter(a_tied.data(), [&](long a) { return a_pp[(size_t)a]; }, tied_out, [&](long s) { return pos_ptr[s]; });
    X.scatter(a_nan.data(), one, nan_out, one);
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
    if (kind == 0 && rank_eval_prefilter_) {   // section 6aj: rows of RANK_EVAL_MX_POS positives in units of 64, the matrix rule over them
        long nrow = units, piece = 0;
        if (pos_ptr) {
            check(pos_ptr[0] >= 0, "rank_geometry: pos_ptr must start at >= 0");
            for (long s = 0; s < units; s++) check(pos_ptr[s + 1] >= pos_ptr[s], "rank_geometry: pos_ptr must not decrease");
            piece = rank_eval_piece(0, units, rank_eval_budget_, [&](long s) {
                return pos_ptr[s + 1] - pos_ptr[s] + 1 + rank_eval_band_cost(pos_ptr[s + 1] - pos_ptr[s], rank_eval_band_, RANK_EVAL_MX_POS);
            });
            RankEvalRows rows;
            rank_eval_rows(pos_ptr, 0, piece, 64, RANK_EVAL_MX_POS, rows);
            nrow = rows.nrow();
        }
        if (nrow > 0) rank_topn_geometry(P, nrow, LONG_MAX, &gy, &per, 1);
        out[2] = rank_eval_band_; out[3] = 64; out[4] = nrow; out[5] = (nrow + 63) / 64; out[6] = piece; out[7] = nrow > 0 ? 1 : 0;
    } else if (kind == 0) {
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
        rank_topn_admit("rank_geometry", top_n, "");
        // the prefilter (section 6ai) acts while rank_topn_scores is 0, and on no deep call (section 6al): the matrix rule at top_n + slack
        const bool deep = top_n > RANK_TOPN_MAX, prefilter = rank_topn_prefilter_ && !rank_topn_scores_ && !deep;
        const int matrix = rank_topn_scores_ || prefilter;
        const int cap = deep ? rank_topn_deep_cap(top_n) : rank_topn_cap(P, prefilter ? top_n + rank_topn_slack_ : top_n, matrix);
        const long max_lists = std::max<long>(1, rank_topn_budget_ / cap);
        const std::vector<int64_t> no_bans((size_t)units + 1, 0);
        const long piece = rank_topn_piece(0, units, max_lists, no_bans);   // units sections without bans: the first piece
        rank_topn_geometry(P, piece, max_lists, &gy, &per, matrix);
        const long ts = rank_topn_tile_rows(P, matrix);
        out[2] = cap; out[3] = ts; out[4] = piece; out[5] = (piece + ts - 1) / ts; out[6] = piece; out[7] = 1;
    }
    out[0] = gy; out[1] = per;
}

}  // namespace svdf

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
#include "svdf_rankrows_lists.h"

namespace svdf {

void Engine::rank_cand(const char *who, long S, RankRowSource R, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *cand_ptr,
                       const unsigned *cand_item, int top_n, int *position_out, int *tied_out, int *ranked_out, int *item_out, float *score_out,
                       int *count_out, int *nan_out) {
    const std::string w(who);
    const bool topn = !strcmp(who, "rank_topn");
    if ((R.user != nullptr) == (R.lines.ptr != nullptr)) fail(w + ": give the sections either as users or as USER lines");
    // what the twin refuses: with users the _fb call's configurations (a format_type = 0 trainer without lists: the plain call's), with
    // USER lines the _lines call's
    if (!rank_live_fb_refusals(who, R.fb.ptr != nullptr, R.lines.ptr != nullptr)) R.fb = RankList();
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
    if (R.user)
        for (long s = 0; s < S; s++) check(R.user[s] < (unsigned)mp_.num_user, "user feature index exceed bound");
    RankCandLists L;
    // knob rank_cand_build = 1: the device builds the sets (section 6ak).  What rank_cand_build refuses about the positives is refused here;
    // raw_first counts a section's raw ids, candidates + positives, which bound its set: the pieces are cut on them
    const bool dev_asked = rank_cand_build_ == 1;
    bool dev = dev_asked;
    std::vector<int64_t> raw_first;
    std::vector<int> dev_ranked;
    if (dev) {
        if (pos_ptr) rank_cand_check_positives(S, pos_ptr, pos_item, (long)mp_.num_item);
        raw_first.assign((size_t)S + 1, 0);
        dev_ranked.assign((size_t)S, 0);
        for (long s = 0; s < S; s++) {
            const int64_t n = cand_ptr[s + 1] - cand_ptr[s] + (pos_ptr ? pos_ptr[s + 1] - pos_ptr[s] : 0);
            if (!rank_cand_set_form(n, (int64_t)mp_.num_item, (int)rank_cand_build_form_)) dev = false;   // one section neither form takes: the whole call
            raw_first[(size_t)s + 1] = raw_first[(size_t)s] + n;
        }
    }
    if (!dev) {
        // long calls build their sets on several host threads (sort + unique is the call's largest host part: profiles/r31_rank_cand.md)
        const int64_t entries = S > 0 ? cand_ptr[S] - cand_ptr[0] : 0;
        const int threads = entries < (1 << 18) ? 1 : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        rank_cand_build(S, cand_ptr, cand_item, pos_ptr, pos_item, (long)mp_.num_item, L, threads);
    }
    rank_rows_validate(who, S, R);
    for (long s = 0; s < S; s++) {
        nan_out[s] = 0;
        if (topn) count_out[s] = 0;
        else ranked_out[s] = dev ? 0 : L.ranked[(size_t)s];
    }
    need_device(who);
    if (dev_asked && !dev) n_rank_cand_host_++;
    // (under the device build a positions call without any positive still builds the sets: ranked_out comes from them)
    if (S == 0 || (!dev && !topn && pos_ptr[S] == pos_ptr[0])) return;
    flush();   // behind whatever has been staged
    const std::vector<int64_t> &first = dev ? raw_first : L.first;   // what the pieces are cut on
    const int *ranked = dev ? dev_ranked.data() : L.ranked.data();
    const DevParams &P = params();
    if (R.lines.ptr) rank_live_items(who, R);   // once per call: the whole catalogue, whatever the lists name
    const int N = top_n;
    const int64_t *extra[3] = {pos_ptr, R.fb.ptr, R.lines.ptr};
    std::vector<int> in, back, tile_q0, tile_sec, sizes;
    std::vector<int64_t> dense;
    for (long s0 = 0; s0 < S;) {
        // ---- a piece of whole sections within the entry budget
        const long s1 = rank_cand_piece(who, s0, S, first, extra, 3, rank_eval_budget_);
        const long nsec = s1 - s0;
        const int64_t npos = topn ? 0 : pos_ptr[s1] - pos_ptr[s0];
        check(npos < INT_MAX / 4 && (!R.fb.ptr || R.fb.ptr[s1] - R.fb.ptr[s0] < INT_MAX / 4) && (!R.lines.ptr || R.lines.ptr[s1] - R.lines.ptr[s0] < INT_MAX / 4),
              (w + ": one section with more than 2^29 entries").c_str());
        if (!dev && !topn && npos == 0) { s0 = s1; continue; }
        auto put = [&in](size_t n) { const size_t at = in.size(); in.resize(at + n); return at; };
        // what the kernels read, wherever the piece's build has put it
        int64_t npair = 0;
        int ntile = 0;
        const int *d_in, *d_user, *d_q0, *d_id, *d_tq0, *d_tsec, *d_p0 = nullptr, *d_at = nullptr, *d_flag = nullptr;
        RankRowsAt o_rows;   // the row lists end either build's first upload, d_in
        if (!dev) {
            npair = L.first[(size_t)s1] - L.first[(size_t)s0];
            rank_cand_tiles(s0, s1, L.first, tile_q0, tile_sec);
            ntile = (int)tile_sec.size();
            // ---- one upload: sec_user | sec_q0 | cand_id | tile_q0 | tile_sec [| sec_p0 | pos_at] [| fb_p0 | fb_index | fb_value] [| ul_p0 | ul_index | ul_value]
            in.clear();
            in.reserve(2 * (size_t)nsec + 1 + (size_t)npair + 2 * (size_t)ntile + 1 + (topn ? 0 : (size_t)nsec + 1 + (size_t)npos) +
                       rank_rows_words(R, s0, s1));
            const size_t o_user = put((size_t)nsec), o_q0 = put((size_t)nsec + 1), o_id = put((size_t)npair);
            for (long s = s0; s <= s1; s++) {
                if (s < s1) in[o_user + (size_t)(s - s0)] = R.user_of(s);   // (with lines the rows do not read it)
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
            o_rows = rank_rows_pack(R, s0, s1, in);
            reserve_or_fail(who, ca_in_, in.size(), "the lists of a piece");
            ca_in_.upload(in.data(), in.size(), stream_);
            d_in = ca_in_.p;
            d_user = ca_in_.p + o_user; d_q0 = ca_in_.p + o_q0; d_id = ca_in_.p + o_id;
            d_tq0 = ca_in_.p + o_tq0; d_tsec = ca_in_.p + o_tsec;
            d_p0 = ca_in_.p + o_p0; d_at = ca_in_.p + o_at;
        } else {
            // ---- the device build.  One upload: sec_user | sec_r0 | sec_form | set_size | flag | the raw ids, per section its candidates, then
            // its positives [| sec_p0 | pos_id] [| fb ...] [| ul ...]
            const int64_t nraw = raw_first[(size_t)s1] - raw_first[(size_t)s0];
            in.clear();
            in.reserve(4 * (size_t)nsec + 2 + (size_t)nraw + (topn ? 0 : (size_t)nsec + 1 + (size_t)npos) +
                       rank_rows_words(R, s0, s1));
            const size_t o_user = put((size_t)nsec), o_r0 = put((size_t)nsec + 1), o_form = put((size_t)nsec), o_size = put((size_t)nsec), o_flag = put(1),
                         o_raw = put((size_t)nraw);
            in[o_flag] = 0;
            int lds_words = 64;
            int64_t by_form[3] = {0, 0, 0};
            for (long s = s0; s < s1; s++) {
                const size_t q = (size_t)(s - s0);
                const int64_t n = raw_first[(size_t)s + 1] - raw_first[(size_t)s];
                const int form = rank_cand_set_form(n, (int64_t)mp_.num_item, (int)rank_cand_build_form_);
                in[o_user + q] = R.user_of(s);
                in[o_r0 + q] = (int)(raw_first[(size_t)s] - raw_first[(size_t)s0]);
                in[o_form + q] = form;
                in[o_size + q] = 0;
                by_form[form]++;
                lds_words = std::max(lds_words, rank_cand_sets_lds_words(n, (int64_t)mp_.num_item, form));
                int *at = in.data() + o_raw + (size_t)in[o_r0 + q];
                if (cand_ptr[s + 1] > cand_ptr[s]) at = std::copy(cand_item + cand_ptr[s], cand_item + cand_ptr[s + 1], at);
                if (!topn && pos_ptr[s + 1] > pos_ptr[s]) std::copy(pos_item + pos_ptr[s], pos_item + pos_ptr[s + 1], at);
            }
            in[o_r0 + (size_t)nsec] = (int)nraw;
            size_t o_p0 = 0, o_pid = 0;
            if (!topn) {
                o_p0 = put((size_t)nsec + 1);
                o_pid = put((size_t)npos);
                for (long s = s0; s <= s1; s++) in[o_p0 + (size_t)(s - s0)] = (int)(pos_ptr[s] - pos_ptr[s0]);
                if (npos > 0) std::copy(pos_item + pos_ptr[s0], pos_item + pos_ptr[s1], in.begin() + (long)o_pid);
            }
            o_rows = rank_rows_pack(R, s0, s1, in);
            reserve_or_fail(who, cb_in_, in.size(), "the lists of a piece");
            cb_in_.upload(in.data(), in.size(), stream_);
            // ---- the sets, in place; their sizes come back: the host needs them for ranked_out, the dense offsets and the tile table
            RankCandSetsDev B;
            B.nsec = (int)nsec;
            B.num_item = (unsigned)mp_.num_item;
            B.sec_r0 = cb_in_.p + o_r0; B.sec_form = cb_in_.p + o_form;
            B.raw = cb_in_.p + o_raw; B.set_size = cb_in_.p + o_size;
            B.lds_words = lds_words;
            launch_rank_cand_sets(B, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            sizes.resize((size_t)nsec);
            HIPCHECK(hipMemcpyAsync(sizes.data(), B.set_size, (size_t)nsec * sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
            n_rank_cand_sort_ += by_form[1];
            n_rank_cand_bitmap_ += by_form[2];
            dense.assign((size_t)nsec + 1, 0);
            for (long s = s0; s < s1; s++) {
                const size_t q = (size_t)(s - s0);
                check(sizes[q] >= 0 && sizes[q] <= in[o_r0 + q + 1] - in[o_r0 + q], (w + ": internal error: a section's set is larger than its lists").c_str());
                dev_ranked[(size_t)s] = sizes[q];
                if (!topn) ranked_out[s] = sizes[q];
                // in a positions call only the sections WITH positives are kept, as in rank_cand_build
                dense[q + 1] = dense[q] + (topn || pos_ptr[s + 1] > pos_ptr[s] ? sizes[q] : 0);
            }
            if (!topn && npos == 0) { s0 = s1; continue; }
            npair = dense[(size_t)nsec];
            rank_cand_tiles(0, nsec, dense, tile_q0, tile_sec);
            ntile = (int)tile_sec.size();
            // ---- the second upload, a few words: sec_q0 | tile_q0 | tile_sec; behind them k_rank_cand_pack's cand_id | pos_at
            in.clear();
            const size_t o_q0 = put((size_t)nsec + 1), o_tq0 = put((size_t)ntile + 1), o_tsec = put((size_t)ntile);
            for (long q = 0; q <= nsec; q++) in[o_q0 + (size_t)q] = (int)dense[(size_t)q];
            std::copy(tile_q0.begin(), tile_q0.end(), in.begin() + (long)o_tq0);
            std::copy(tile_sec.begin(), tile_sec.end(), in.begin() + (long)o_tsec);
            const size_t o_id = in.size(), o_at = o_id + (size_t)npair;
            reserve_or_fail(who, ca_in_, o_at + (size_t)npos, "the sets of a piece");
            ca_in_.upload(in.data(), in.size(), stream_);
            B.sec_q0 = ca_in_.p + o_q0;
            B.cand_id = ca_in_.p + o_id;
            if (!topn) { B.sec_p0 = cb_in_.p + o_p0; B.pos_id = cb_in_.p + o_pid; B.pos_at = ca_in_.p + o_at; }
            B.flag = cb_in_.p + o_flag;
            launch_rank_cand_pack(B, stream_);
            HIPCHECK(hipGetLastError());
            n_launches_++;
            d_user = cb_in_.p + o_user; d_q0 = B.sec_q0; d_id = B.cand_id;
            d_tq0 = ca_in_.p + o_tq0; d_tsec = ca_in_.p + o_tsec;
            d_p0 = B.sec_p0; d_at = B.pos_at; d_flag = B.flag;
            d_in = cb_in_.p;
        }
        // ---- the workspaces: the pairs' scores; position | tied | nan, or nan | count | items | scores
        const size_t nres = topn ? (size_t)nsec * (2 + 2 * (size_t)N) : 2 * (size_t)npos + (size_t)nsec;
        reserve_or_fail(who, ca_score_, (size_t)npair, "the candidate scores of a piece");
        reserve_or_fail(who, ca_out_, nres, "the results of a piece");
        RankCandDev D;
        D.nsec = (int)nsec;
        D.sec_user = reinterpret_cast<const unsigned *>(d_user);
        D.item_rows = R.item_rows; D.item_bias = R.item_bias;
        D.user_rows = rank_rows_launch(who, R, d_in, o_rows, D.sec_user, s0, s1);
        D.sec_q0 = d_q0;
        D.cand_id = d_id;
        D.cand_score = ca_score_.p;
        D.ntile = ntile;
        D.tile_q0 = d_tq0; D.tile_sec = d_tsec;
        D.top_n = N;
        if (topn) {
            D.nan_out = ca_out_.p; D.count_out = D.nan_out + nsec; D.item_out = D.count_out + nsec;
            D.score_out = reinterpret_cast<float *>(D.item_out + (size_t)nsec * N);
        } else {
            D.npos = (long)npos;
            D.sec_p0 = d_p0; D.pos_at = d_at;
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
                check(b_cnt[q] == (bad ? 0 : std::min(N, ranked[(size_t)s])), "rank_topn: internal error: a section's list is not as long as its candidates allow");
                nan_out[s] = bad ? 1 : 0;
                count_out[s] = b_cnt[q];
            }
            n_rank_topn_sections_ += nsec;
            n_rank_cand_sections_ += nsec;
            if (R.fb.ptr) n_rank_fb_sections_ += nsec;
            if (R.lines.ptr) n_rank_line_sections_ += nsec;
        } else {
            back.resize(nres);
            HIPCHECK(hipMemcpyAsync(back.data(), ca_out_.p, nres * sizeof(int), hipMemcpyDeviceToHost, stream_));
            int lost = 0;   // the device build: k_rank_cand_pack found a positive in no set
            if (d_flag) HIPCHECK(hipMemcpyAsync(&lost, d_flag, sizeof(int), hipMemcpyDeviceToHost, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
            check(lost == 0, "rank_eval: internal error: a positive is not in its section's set");
            n_rank_cand_sections_ += rank_positions_back(R, pos_ptr, s0, s1, back.data(), back.data() + npos, back.data() + 2 * npos, position_out,
                                                         tied_out, nan_out);
        }
        s0 = s1;
    }
}

}  // namespace svdf

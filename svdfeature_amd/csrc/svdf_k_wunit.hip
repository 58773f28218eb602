// svdf_k_wunit.hip -- the WINDOW-MINIBATCH step for user units: user-group (SVD++) blocks and rows with global features
// (part of the gfx950 kernel set described at the top of svdf_device.h).
//
// Exact sequential semantics leave these shapes a handful of users per launch (BASELINE configs[3]: ~6 SVD++ users or ~280 neighbourhood
// rows per conflict-free level), because every instance reads and writes SHARED rows: W_item / i_bias, the implicit-feedback rows
// W_ufeedback / ufeedback_bias (apex_svd_base.h:523-554) and the global biases (:188-210, :313-353).  The window step defers exactly those:
//   * a user's unit runs exact on its PRIVATE state -- its W_user row and bias and, for SVD++, tmp_ufeedback / old_ufeedback
//     (SVDPPFeature's members, :486-488) -- instance after instance in file order, one lane group per user: k_wunit_walk;
//   * the shared rows are read as they were at the window start (nothing writes them inside a window: they are their own snapshot) and
//     what the reference WOULD have changed on them -- (q + s p) decay - q per item entry, reg(g + s) - g per global entry,
//     (w + d val) - w per feedback row at the unit's end -- goes to a contribution slot;
//   * k_wunit_sum adds every shared row's contributions IN FILE ORDER (slots are laid out target by target; no float atomics: the result
//     is deterministic and equals oracle/svdf_oracle.c: svdo_update_block_stale / svdo_update_csr_batch_stale bit for bit) and either adds
//     the sum to the model in place (one GPU, `amd:step = minibatch`) or writes the wire buffer of the N-rank exchange.
#include <algorithm>
#include <cstdlib>
#include <stdexcept>

#include "svdf_instance.h"

namespace svdf {

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------- kernel A: the users' exact walks
// FB: the trainer is SVDPPFeature (user-group format): a segment prepares tmp_ufeedback from its feedback list (:523-538), every row
// goes through the update_svdpp hook (:512-520), the segment's end is update_ufeedback (:539-554) against the window-start rows.
// General form: any width, any row shape (one user entry per row), every link and regulariser of the base solver.  R: the row type -- float4 (one lane
// group per unit, num_factor <= 256) or WideRow<2..4> (LPI = 64: one wave per unit, HOT = false only).
// Shared user rows (S.uptr, amd:shared_user_from): the row's other user entries are read as of the window start, in entry order around the
// private one (calc_bias :313-353, prepare_tmp :354-381), and their change goes to a contribution slot like an item row's.
// Side-table children: feature_user children are shared user entries (the builder expands them); feature_item children
// (S.iptr) follow their parent entry in every loop, with the reference's item-side forms for parent value ival and child value v: bias term
// (b v) ival, tmp_i scale (float)((double)v ival), update scale ((lr err) v) ival -- svdf_instance.h restates the same forms for the exact pass.
// HOT: the window has hot shared user rows or hot item rows (ordered sub-steps, kernel C below); windows without them run the HOT = false build, the
// code as it was.  FB and HOT together: user-group windows with hot shared user rows (knob window_block_sub) or hot item rows
// (knob window_block_item_sub, section 6u).
template <int LPI, bool FB, bool HOT = false, typename R = float4>
__global__ __launch_bounds__(256) void k_wunit_walk(const DevParams P, const WUnitSchedule S) {
    using io = row_io<LPI, R>;
    using cio = contrib_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63;
    const int L = lane & (LPI - 1);
    const long uidx = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW + lane / LPI;
    if (uidx >= S.nunits) return;
    const WinUnit un = S.units[uidx];
    const int pitch = P.pitch, k = P.k;
    const bool ub = P.no_user_bias == 0;
    const float lr = P.lr;
    const unsigned ur = P.user_off + un.user;
    R p = io::load(P.W, ur, pitch, L, k);
    float bu = ub ? P.bias[ur] : 0.0f;
    const float wd_u = get_wd(P.u_rng, un.user, P.wd_user);
    for (int sg = 0; sg < un.seg_count; sg++) {
        const WinSeg seg = sg == 0 ? un.first : S.segs[un.seg_begin + sg];
        SvdppRegsT<R> pp;
        pp.tmp_fb = row_traits<R>::zero(); pp.old_fb = row_traits<R>::zero(); pp.norm = 0.0f; pp.tmp_bias = 0.0f; pp.old_bias = 0.0f;
        if (FB) {   // prepare_ufeedback + the backup of update(block) (:568-574)
            for (int j = seg.fb_begin; j < seg.fb_begin + seg.fb_count; j++) {
                const WinEnt f = S.fbent[j];
                const unsigned row = P.fb_off + f.idx;
                axpy4(pp.tmp_fb, io::load(P.W, row, pitch, L, k), f.val);
                pp.norm = pp.norm + f.val * f.val;
                if (ub) pp.tmp_bias = pp.tmp_bias + P.bias[row] * f.val;
            }
            pp.old_bias = pp.tmp_bias;
            pp.old_fb = pp.tmp_fb;
        }
        for (int r = seg.row_begin; r < seg.row_begin + seg.row_count; r++) {
            int e0, e1, e2;
            if (S.rptr) { e0 = S.rptr[2 * (long)r]; e1 = S.rptr[2 * (long)r + 1]; e2 = S.rptr[2 * (long)r + 2]; }
            else { e0 = r * S.estride; e1 = e0 + S.estride - 1; e2 = e1 + 1; }
            const float label = S.label[r];
            const float ua = S.uval ? S.uval[r] : 1.0f;
            int u0 = 0, um = 0, u1 = 0;   // shared user entries: [u0, um) before the private one, [um, u1) after it
            if (S.uptr) { u0 = S.uptr[r]; um = u0 + S.upos[r]; u1 = S.uptr[r + 1]; }
            int c0 = 0, c1 = 0;           // feature_item children: [c0, c1), parent by parent (ient.pad = the parent's entry)
            if (S.iptr) { c0 = S.iptr[r]; c1 = S.iptr[r + 1]; }
            const size_t srow0 = (size_t)P.user_off + S.shared_from;
            // ---- pred (:445-454): calc_bias in double, the hooks' terms where the reference adds them
            double bs = 0.0;
            for (int j = e0; j < e1; j++) { const WinEnt e = S.ent[j]; bs += (double)(e.val * P.g_bias[e.idx]); }
            if (ub) {
                for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * P.bias[srow0 + e.idx]); }
                bs += (double)(ua * bu);
                for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * P.bias[srow0 + e.idx]); }
                bs += (double)(FB ? pp.tmp_bias : 0.0f);
            }
            bs += 0.0;
            for (int j = e1, c = c0; j < e2; j++) {
                const WinEnt e = S.ent[j];
                bs += (double)(e.val * P.bias[P.item_off + e.idx]);
                for (; c < c1 && S.ient[c].pad == j; c++) { const WinEnt ch = S.ient[c]; bs += (double)(P.bias[P.item_off + ch.idx] * ch.val * e.val); }
            }
            double sum = (double)P.base_score + bs;
            R tu = FB ? pp.tmp_fb : row_traits<R>::zero();
            for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; axpy4(tu, io::load(P.W, srow0 + e.idx, pitch, L, k), e.val); }
            axpy4(tu, p, ua);
            for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; axpy4(tu, io::load(P.W, srow0 + e.idx, pitch, L, k), e.val); }
            R ti = row_traits<R>::zero();
            for (int j = e1, c = c0; j < e2; j++) {
                const WinEnt e = S.ent[j];
                axpy4(ti, io::load(P.W, P.item_off + e.idx, pitch, L, k), e.val);
                for (; c < c1 && S.ient[c].pad == j; c++) {   // scalar formed in double
                    const WinEnt ch = S.ient[c];
                    axpy4(ti, io::load(P.W, P.item_off + ch.idx, pitch, L, k), (float)((double)ch.val * (double)e.val));
                }
            }
            sum += (double)group_dot<LPI>(tu, ti, L, k);
            const float pred = map_active((float)sum, P.active_type);
            const float err = cal_grad(label, pred, P.active_type) * 1.0f;
            // ---- update_no_decay (:383-427) + regularize(after) (:286-311), the shared rows' part as contributions
            for (int j = e0; j < e1; j++) {
                const WinEnt e = S.ent[j];
                const float g = P.g_bias[e.idx];
                float g2 = g + lr * err * e.val;
                g2 = reg_gbias(P, e.idx, g2);
                if (L == 0) S.gcontrib[e.slot] = g2 - g;
            }
            const float su = lr * err * ua;
            R wu = p;
            axpy4(wu, ti, su);
            float nbu = bu + su;
            for (int j = e1; j < e2; j++) {
                const WinEnt e = S.ent[j];
                if (HOT && e.pad) {   // a hot item row of this window (k_wunit_apply_hot<ITEM>): the same record as for a hot shared user row below
                    cio::store(S.contrib, 0, (size_t)e.slot, pitch, L, k, p);
                    if (L == 0) S.cbias[e.slot] = bu;
                    if (FB) {   // user-group windows (knob window_block_item_sub, section 6u): the span's feedback state too, as for a hot uent below (pad = 1 + record)
                        cio::store(S.hfb, 0, (size_t)(e.pad - 1), pitch, L, k, pp.tmp_fb);
                        if (L == 0) S.hfbb[e.pad - 1] = pp.tmp_bias;
                    }
                    continue;
                }
                const float si = lr * err * e.val;
                const R q = io::load(P.W, P.item_off + e.idx, pitch, L, k);
                const float bi = P.bias[P.item_off + e.idx];
                R wi = q;
                axpy4(wi, tu, si);
                float nbi = bi + si;
                reg_row<LPI>(P, wi, get_wd(P.i_rng, e.idx, P.wd_item), true, L);
                nbi = nbi * (1.0f - lr * P.wd_item_bias);
                sub4(wi, q);
                if (e.slot < 0) {   // the row's only contribution of this window: applied here (apply_single, svdf_device.h)
                    io::store(P.W, P.item_off + e.idx, pitch, L, k, apply_single(q, wi, S.contrib_bf16 != 0));
                    if (L == 0) P.bias[P.item_off + e.idx] = apply_single(bi, nbi - bi, false);
                } else {
                    cio::store(S.contrib, S.contrib_bf16, (size_t)e.slot, pitch, L, k, wi);
                    if (L == 0) S.cbias[e.slot] = nbi - bi;
                }
            }
            for (int j = e1, c = c0; c < c1; j++) {   // feature_item children: update_no_decay + reg_item against the window-start rows
                const float ival = S.ent[j].val;
                for (; c < c1 && S.ient[c].pad == j; c++) {
                    const WinEnt ch = S.ient[c];
                    if (HOT && ch.slot < -1) {   // a hot child (its slot travels as -2 - slot: ient.pad is taken by the parent's position)
                        cio::store(S.contrib, 0, (size_t)(-2 - ch.slot), pitch, L, k, p);
                        if (L == 0) S.cbias[-2 - ch.slot] = bu;
                        continue;
                    }
                    const float si = lr * err * ch.val * ival;
                    const size_t row = (size_t)P.item_off + ch.idx;
                    const R q = io::load(P.W, row, pitch, L, k);
                    const float bi = P.bias[row];
                    R wi = q;
                    axpy4(wi, tu, si);
                    float nbi = bi + si;
                    reg_row<LPI>(P, wi, get_wd(P.i_rng, ch.idx, P.wd_item), true, L);
                    nbi = nbi * (1.0f - lr * P.wd_item_bias);
                    sub4(wi, q);
                    if (ch.slot < 0) {   // the row's only contribution of this window
                        io::store(P.W, row, pitch, L, k, apply_single(q, wi, false));
                        if (L == 0) P.bias[row] = apply_single(bi, nbi - bi, false);
                    } else {
                        cio::store(S.contrib, 0, (size_t)ch.slot, pitch, L, k, wi);
                        if (L == 0) S.cbias[ch.slot] = nbi - bi;
                    }
                }
            }
            for (int j = u0; j < u1; j++) {   // shared user rows: update_no_decay + reg_user (:211-249) against the window-start row
                const WinEnt e = S.uent[j];
                if (HOT && e.pad) {   // a hot row of this window (ordered sub-steps, k_wunit_apply_shared): the slot takes what only this walk knows --
                               // the private user's row and bias as they are before this data row's update
                    cio::store(S.contrib, 0, (size_t)e.slot, pitch, L, k, p);
                    if (L == 0) S.cbias[e.slot] = bu;
                    if (FB) {   // ... and the span's tmp_ufeedback / tmp_ufeedback_bias likewise, in the record's row of the second plane (pad = 1 + record)
                        cio::store(S.hfb, 0, (size_t)(e.pad - 1), pitch, L, k, pp.tmp_fb);
                        if (L == 0) S.hfbb[e.pad - 1] = pp.tmp_bias;
                    }
                    continue;
                }
                const float ss = lr * err * e.val;
                const size_t row = srow0 + e.idx;
                const R w = io::load(P.W, row, pitch, L, k);
                R ws = w;
                axpy4(ws, ti, ss);
                reg_row<LPI>(P, ws, get_wd(P.u_rng, S.shared_from + e.idx, P.wd_user), false, L);
                sub4(ws, w);
                float cb = 0.0f, b = 0.0f;
                if (ub) { b = P.bias[row]; float nb = b + ss; nb = nb * (1.0f - lr * P.wd_user_bias); cb = nb - b; }
                if (e.slot < 0) {   // the row's only contribution of this window
                    io::store(P.W, row, pitch, L, k, apply_single(w, ws, false));
                    if (ub && L == 0) P.bias[row] = apply_single(b, cb, false);
                } else {
                    cio::store(S.contrib, 0, (size_t)e.slot, pitch, L, k, ws);
                    if (L == 0) S.cbias[e.slot] = cb;
                }
            }
            if (FB) pp.update(P, err, ti, ub);
            reg_row<LPI>(P, wu, wd_u, false, L);
            nbu = nbu * (1.0f - lr * P.wd_user_bias);
            p = wu;
            if (ub) bu = nbu;
        }
        if (FB && seg.fb_count > 0) {   // update_ufeedback (:539-554) against the window-start feedback rows
            R d = pp.tmp_fb;
            sub4(d, pp.old_fb);
            float db = pp.tmp_bias - pp.old_bias;
            const float inv = 1.0f / pp.norm;
            scale4(d, inv);
            db = db * inv;
            if (S.fbrec) {   // deferred scatter: the segment's delta; k_wunit_sum forms (w + d val) - w against the rows it updates
                io::store(S.dvec, (size_t)(un.seg_begin + sg), pitch, L, k, d);   // (raw float4 chunks at L * 4, like a model row)
                if (L == 0) S.dbias[un.seg_begin + sg] = db;
            } else
            for (int j = seg.fb_begin; j < seg.fb_begin + seg.fb_count; j++) {
                const WinEnt f = S.fbent[j];
                const unsigned row = P.fb_off + f.idx;
                const R w = io::load(P.W, row, pitch, L, k);
                R w2 = w;
                axpy4(w2, d, f.val);
                sub4(w2, w);
                if (f.slot < 0) io::store(P.W, row, pitch, L, k, apply_single(w, w2, S.contrib_bf16 != 0));
                else cio::store(S.contrib, S.contrib_bf16, (size_t)f.slot, pitch, L, k, w2);
                if (L == 0) {
                    const float b = (ub || f.slot < 0) ? P.bias[row] : 0.0f;
                    float cb = 0.0f;
                    if (ub) { const float b2 = b + db * f.val; cb = b2 - b; }
                    if (f.slot < 0) P.bias[row] = apply_single(b, cb, false);
                    else S.cbias[f.slot] = cb;
                }
            }
        }
    }
    io::store(P.W, ur, pitch, L, k, p);
    if (ub && L == 0) P.bias[ur] = bu;
}

// ------------------------------------------------------------------------------------------------- kernel A, the BASELINE configs[3] shapes
// Full rows of k = 4 * LANES * V floats (64 / 128) held V chunks per lane by LANES lanes -- 64 / LANES units per wave instead of two --,
// the T = 16 / LANES units of a DPP row interleaved (dot_slots reproduces the reference's four SSE chains, svdf_device.h), fixed row
// layout (NG global entries + one item entry), unit user values, reg_method 0 / 1 / 3 (elementwise).  The arithmetic is the general
// kernel's, statement for statement.  What differs is latency:
//   * NG == 0 (SVD++ and plain rows: LONG units -- 100 rows per user at configs[3]): the shared side is read-only inside a window, so the
//     rows ahead cannot go stale: a ring of D rows is in flight (records two cycles ahead, item rows one cycle ahead), and the feedback
//     gather / scatter requests eight rows at a time.  A window's launch lasts as long as its longest unit: 100 dependent row steps.
//   * NG > 0 (neighbourhood rows: SHORT units, about one row per user and window): D = 1; the gain is units in flight.
__device__ __forceinline__ void reg_chunk(const DevParams &P, float4 &w, float wd, bool is_item) {   // reg_row without the projection mode
    const float lambda = P.lr * wd;
    int method = P.reg_method;
    if (method == 3) method = is_item ? 0 : 1;
    if (method == 0) scale4(w, 1.0f - lambda);
    else l1_row(w, lambda);
    if (!is_item && P.user_nonnegative) clamp_nonneg(w);
}
template <int LANES, int V, bool FB, int NG, int D>
__global__ __launch_bounds__(256) void k_wunit_fast(const DevParams P, const WUnitSchedule S) {
    constexpr int T = 16 / LANES, IPW = 64 / LANES, K = 4 * LANES * V, E = NG + 1;
    static_assert(NG == 0 || D == 1, "the row ring is for rows without global entries");
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int m = (lane & 15) / T;
    const int gslot = (lane >> 4) * T + (lane & (T - 1));
    const long uidx = wave * IPW + gslot;
    if (uidx >= S.nunits) return;
    const WinUnit un = S.units[uidx];
    const int pitch = P.pitch;
    const bool ub = P.no_user_bias == 0;
    const float lr = P.lr;
    const unsigned ur = P.user_off + un.user;
    float4 p[V];
#pragma unroll
    for (int v = 0; v < V; v++) p[v] = load_row_nt<K / 4>(P.W, ur, pitch, m + v * LANES, K);
    float bu = ub ? P.bias[ur] : 0.0f;
    const float wd_u = get_wd(P.u_rng, un.user, P.wd_user);
    const float dec_ub = 1.0f - lr * P.wd_user_bias, dec_ib = 1.0f - lr * P.wd_item_bias;
    for (int sg = 0; sg < un.seg_count; sg++) {
        const WinSeg seg = sg == 0 ? un.first : S.segs[un.seg_begin + sg];
        float4 tmp_fb[V], old_fb[V];
        float norm = 0.0f, tmp_bias = 0.0f, old_bias = 0.0f;
#pragma unroll
        for (int v = 0; v < V; v++) { tmp_fb[v] = f4zero(); old_fb[v] = f4zero(); }
        if (FB) {   // prepare_ufeedback (:523-538), eight rows requested at a time, accumulated in list order
            for (int j0 = 0; j0 < seg.fb_count; j0 += 8) {
                WinEnt f[8];
                float4 w[8][V];
                float b[8];
#pragma unroll
                for (int q = 0; q < 8; q++) f[q] = S.fbent[seg.fb_begin + (j0 + q < seg.fb_count ? j0 + q : j0)];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const unsigned row = P.fb_off + f[q].idx;
#pragma unroll
                    for (int v = 0; v < V; v++) w[q][v] = load_row<K / 4>(P.W, row, pitch, m + v * LANES, K);
                    b[q] = ub ? P.bias[row] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    if (j0 + q < seg.fb_count) {
#pragma unroll
                        for (int v = 0; v < V; v++) axpy4(tmp_fb[v], w[q][v], f[q].val);
                        norm = norm + f[q].val * f[q].val;
                        if (ub) tmp_bias = tmp_bias + b[q] * f[q].val;
                    }
                }
            }
            old_bias = tmp_bias;
#pragma unroll
            for (int v = 0; v < V; v++) old_fb[v] = tmp_fb[v];
        }
        // ---- one row: the general kernel's statements on (p, bu, tmp_fb; the row's record, item row q, item bias bi)
        auto step = [&](float label, const WinEnt (&ge)[NG > 0 ? NG : 1], const float (&gb)[NG > 0 ? NG : 1], const WinEnt &ie, const float4 (&q)[V], float bi) {
            double bs = 0.0;
#pragma unroll
            for (int j = 0; j < NG; j++) bs += (double)(ge[j].val * gb[j]);
            if (ub) {
                bs += (double)(1.0f * bu);
                bs += (double)(FB ? tmp_bias : 0.0f);
            }
            bs += 0.0;
            bs += (double)(ie.val * bi);
            double sum = (double)P.base_score + bs;
            float4 tu[V], ti[V];
#pragma unroll
            for (int v = 0; v < V; v++) {
                tu[v] = FB ? tmp_fb[v] : f4zero();
                axpy4(tu[v], p[v], 1.0f);
                ti[v] = f4zero();
                axpy4(ti[v], q[v], ie.val);
            }
            sum += (double)dot_slots<LANES, V>(tu, ti, m, lane);
            const float pred = map_active((float)sum, P.active_type);
            const float err = cal_grad(label, pred, P.active_type) * 1.0f;
#pragma unroll
            for (int j = 0; j < NG; j++) {
                float g2 = gb[j] + lr * err * ge[j].val;
                g2 = reg_gbias(P, ge[j].idx, g2);
                if (m == 0) S.gcontrib[ge[j].slot] = g2 - gb[j];
            }
            const float su = lr * err * 1.0f;
            float nbu = bu + su;
            const float si = lr * err * ie.val;
            float nbi = bi + si;
            nbi = nbi * dec_ib;
            const float wd_i = get_wd(P.i_rng, ie.idx, P.wd_item);
#pragma unroll
            for (int v = 0; v < V; v++) {
                float4 wi = q[v];
                axpy4(wi, tu[v], si);
                reg_chunk(P, wi, wd_i, true);
                sub4(wi, q[v]);
                if (ie.slot < 0) store_row<K / 4>(P.W, P.item_off + ie.idx, pitch, m + v * LANES, K, apply_single(q[v], wi, S.contrib_bf16 != 0));   // the row's only contribution of the window
                else store_contrib<K / 4>(S.contrib, S.contrib_bf16, (size_t)ie.slot, pitch, m + v * LANES, K, wi);
            }
            if (m == 0) {
                if (ie.slot < 0) P.bias[P.item_off + ie.idx] = apply_single(bi, nbi - bi, false);
                else S.cbias[ie.slot] = nbi - bi;
            }
            if (FB) {   // update_svdpp (:512-520)
                const float lr2 = lr * P.scale_lr_ufeedback;
#pragma unroll
                for (int v = 0; v < V; v++) { axpy4(tmp_fb[v], ti[v], lr2 * err * norm); scale4(tmp_fb[v], 1.0f - lr2 * P.wd_ufeedback); }
                if (ub) {
                    tmp_bias = tmp_bias + lr2 * err * norm;
                    tmp_bias = tmp_bias * (1.0f - lr2 * P.wd_ufeedback_bias);
                }
            }
#pragma unroll
            for (int v = 0; v < V; v++) {
                float4 wu = p[v];
                axpy4(wu, ti[v], su);
                reg_chunk(P, wu, wd_u, false);
                p[v] = wu;
            }
            nbu = nbu * dec_ub;
            if (ub) bu = nbu;
        };
        const int n = seg.row_count, r0 = seg.row_begin;
        if constexpr (NG == 0 && D > 1) {
            // rows r0 + j: the entry index IS the row index (estride 1).  rec = this cycle's records, nrec = the next cycle's, q / bi = this
            // cycle's item rows; slot d is refilled right after its row was computed, so a row load has D row steps to arrive
            float lab[D], nlab[D], bi[D];
            WinEnt rec[D], nrec[D];
            float4 q[D][V];
#pragma unroll
            for (int d = 0; d < D; d++) {
                const int r = r0 + (d < n ? d : 0);
                rec[d] = S.ent[r]; lab[d] = S.label[r];
            }
#pragma unroll
            for (int d = 0; d < D; d++) {
                const unsigned row = P.item_off + rec[d].idx;
#pragma unroll
                for (int v = 0; v < V; v++) q[d][v] = load_row<K / 4>(P.W, row, pitch, m + v * LANES, K);
                bi[d] = P.bias[row];
            }
#pragma unroll
            for (int d = 0; d < D; d++) {
                const int r = r0 + (d + D < n ? d + D : 0);
                nrec[d] = S.ent[r]; nlab[d] = S.label[r];
            }
            const WinEnt none[1] = {WinEnt{0u, 0.0f, 0, 0}};
            const float nog[1] = {0.0f};
            for (int base = 0; base < n; base += D) {
#pragma unroll
                for (int d = 0; d < D; d++) {
                    const int j = base + d;
                    if (j < n) {
                        step(lab[d], none, nog, rec[d], q[d], bi[d]);
                        rec[d] = nrec[d]; lab[d] = nlab[d];
                        const unsigned row = P.item_off + rec[d].idx;
#pragma unroll
                        for (int v = 0; v < V; v++) q[d][v] = load_row<K / 4>(P.W, row, pitch, m + v * LANES, K);
                        bi[d] = P.bias[row];
                        const int r = r0 + (j + 2 * D < n ? j + 2 * D : 0);
                        nrec[d] = S.ent[r]; nlab[d] = S.label[r];
                    }
                }
            }
        } else {
            for (int j = 0; j < n; j++) {
                const int r = r0 + j;
                WinEnt ge[NG > 0 ? NG : 1];
                float gb[NG > 0 ? NG : 1];
                ge[0] = WinEnt{0u, 0.0f, 0, 0}; gb[0] = 0.0f;
#pragma unroll
                for (int g = 0; g < NG; g++) ge[g] = S.ent[(long)r * E + g];
                const WinEnt ie = S.ent[(long)r * E + NG];
                const float label = S.label[r];
#pragma unroll
                for (int g = 0; g < NG; g++) gb[g] = P.g_bias[ge[g].idx];
                float4 q[V];
                const unsigned row = P.item_off + ie.idx;
#pragma unroll
                for (int v = 0; v < V; v++) q[v] = load_row<K / 4>(P.W, row, pitch, m + v * LANES, K);
                const float bi = P.bias[row];
                step(label, ge, gb, ie, q, bi);
            }
        }
        if (FB && seg.fb_count > 0) {   // update_ufeedback (:539-554) against the window-start feedback rows, eight rows at a time
            float4 d[V];
#pragma unroll
            for (int v = 0; v < V; v++) { d[v] = tmp_fb[v]; sub4(d[v], old_fb[v]); }
            float db = tmp_bias - old_bias;
            const float inv = 1.0f / norm;
#pragma unroll
            for (int v = 0; v < V; v++) scale4(d[v], inv);
            db = db * inv;
            if (S.fbrec) {   // deferred scatter (see k_wunit_walk)
#pragma unroll
                for (int v = 0; v < V; v++) *reinterpret_cast<float4 *>(S.dvec + (size_t)(un.seg_begin + sg) * pitch + (size_t)(m + v * LANES) * 4) = d[v];
                if (m == 0) S.dbias[un.seg_begin + sg] = db;
            } else
            for (int j0 = 0; j0 < seg.fb_count; j0 += 8) {
                WinEnt f[8];
                float4 w[8][V];
                float b[8];
#pragma unroll
                for (int q = 0; q < 8; q++) f[q] = S.fbent[seg.fb_begin + (j0 + q < seg.fb_count ? j0 + q : j0)];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const unsigned row = P.fb_off + f[q].idx;
#pragma unroll
                    for (int v = 0; v < V; v++) w[q][v] = load_row<K / 4>(P.W, row, pitch, m + v * LANES, K);
                    b[q] = ub ? P.bias[row] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    if (j0 + q < seg.fb_count) {
#pragma unroll
                        for (int v = 0; v < V; v++) {
                            float4 w2 = w[q][v];
                            axpy4(w2, d[v], f[q].val);
                            sub4(w2, w[q][v]);
                            if (f[q].slot < 0) store_row<K / 4>(P.W, P.fb_off + f[q].idx, pitch, m + v * LANES, K, apply_single(w[q][v], w2, S.contrib_bf16 != 0));
                            else store_contrib<K / 4>(S.contrib, S.contrib_bf16, (size_t)f[q].slot, pitch, m + v * LANES, K, w2);
                        }
                        if (m == 0) {
                            float cb = 0.0f;
                            if (ub) { const float b2 = b[q] + db * f[q].val; cb = b2 - b[q]; }
                            if (f[q].slot < 0) { const float b0 = ub ? b[q] : P.bias[P.fb_off + f[q].idx]; P.bias[P.fb_off + f[q].idx] = apply_single(b0, cb, false); }
                            else S.cbias[f[q].slot] = cb;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; v++) store_row<K / 4>(P.W, ur, pitch, m + v * LANES, K, p[v]);
    if (ub && m == 0) P.bias[ur] = bu;
}

// ------------------------------------------------------------------------------------------------- kernel B: per-target sums
// Target t = replicated row t of [W_ufeedback rows | W_item rows]; its contributions sit in slots [tptr[t], tptr[t + 1]) in file order.
// One lane group per target adds them in that order (acc = 0 + c_1 + c_2 ..., eight rows requested at a time).
//   LOCAL: the sum is added to the model in place (one GPU: nobody else holds a part of it);
//   else:  the wire buffer of the exchange, dst = [T rows of `pitch` | T biases | nglobal global biases] (the packed layout of
//          Engine::delta_ranges for the whole item range), fp32 or fp16.
// The global biases' sums (gptr over gcontrib) are taken by the same launch, one thread per global id.
// R: the row type -- float4, or WideRow<2..4> at LPI = 64 for the in-place sums of wide rows (LOCAL, no hot rows): a wave per target
template <int LPI, bool HALF, bool LOCAL, bool HOT = false, typename R = float4>   // HOT: the touched list may hold hot shared user rows / hot item rows (in-place sums only)
__global__ __launch_bounds__(256) void k_wunit_sum(const WUnitSchedule S, float *W, float *bias, float *g_bias, unsigned fb_off, unsigned item_off,
                                                   unsigned user_off, int pitch, int k, void *dst) {
    static_assert(LOCAL || row_traits<R>::VPL == 1, "the wire buffer builds are for float4 rows");
    using io = row_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63;
    const int L = lane & (LPI - 1);
    const long stride = (long)gridDim.x * (blockDim.x >> 6) * IPW;
    const long first = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW + lane / LPI;
    const long T = S.nfb_rows + S.nitem_rows + (LOCAL ? S.nshared_rows : 0);   // shared user rows: one-GPU windows only (in place)
    // a target is a chain of dependent loads (its slot range, the records or rows of its slots, for deferred feedback rows the segments' deltas) and the
    // kernel is bound by how many such chains the resident waves hold, not by bytes: the next target's slot range is requested one iteration ahead
    // One-GPU windows bring the list of targets that have slots (a window touches a fraction of the rows, and a row's only contribution has been applied by
    // the walk): every lane group of a wave then has work in every iteration.
    const bool compact = LOCAL && S.touched != nullptr;
    const long N = compact ? S.ntouched : T;
    long pt = first;
    int pb = 0, pe = 0;
    auto request = [&](long i) {
        if (compact) { const WinTouched x = S.touched[i]; pt = x.t; pb = x.b; pe = x.e; }
        else { pt = i; pb = S.tptr[i]; pe = S.tptr[i + 1]; }
    };
    if (first < N) request(first);
    for (long i = first; i < N; i += stride) {
        const long t = pt;
        const int b = pb, e = pe;
        if (i + stride < N) request(i + stride);
        if (LOCAL && b == e) continue;
        if (HOT && LOCAL && e < 0) {   // a hot shared user row or item row (WinTouched): k_wunit_apply_hot left the row and bias it ends the window with in slot b
            const long ts = t - S.nfb_rows - S.nitem_rows;
            const size_t row = ts < 0 ? (size_t)item_off + (size_t)(t - S.nfb_rows) : (size_t)user_off + S.shared_from + (size_t)ts;
            io::store(W, row, pitch, L, k, io::load(S.contrib, (size_t)b, pitch, L, k));
            if (L == 0 && (ts < 0 || S.user_bias)) bias[row] = S.cbias[b];
            continue;
        }
        R acc = row_traits<R>::zero();
        float accb = 0.0f;
        if (S.fbrec && t < S.nfb_rows) {
            // deferred feedback scatter: slot s names a segment and the entry's value; the contribution is what the unit's walk would have stored --
            // (w + d val) - w against the window-start row, rounded like a stored contribution row -- and the sum runs in slot (= file) order
            const size_t row = (size_t)fb_off + (size_t)t;
            const R w = io::load(W, row, pitch, L, k);
            const float bw = S.user_bias ? bias[row] : 0.0f;
            const bool bf = S.contrib_bf16 != 0;
            constexpr int DB = 4;   // records / deltas requested together (a feedback row of the configs[3] windows meets 1.5 contributions on average)
            for (int s0 = b; s0 < e; s0 += DB) {
                WinFbRec r[DB];
                R d[DB];
                float dbv[DB];
#pragma unroll
                for (int q = 0; q < DB; q++) r[q] = S.fbrec[min(s0 + q, e - 1)];
#pragma unroll
                for (int q = 0; q < DB; q++) {
                    d[q] = io::load(S.dvec, (size_t)r[q].seg, pitch, L, k);
                    dbv[q] = S.dbias[r[q].seg];
                }
#pragma unroll
                for (int q = 0; q < DB; q++) {
                    if (s0 + q < e) {
                        R w2 = w;
                        axpy4(w2, d[q], r[q].val);
                        sub4(w2, w);
                        add_rows(acc, contrib_as_stored(w2, bf));
                        float cb = 0.0f;
                        if (S.user_bias) { const float b2 = bw + dbv[q] * r[q].val; cb = b2 - bw; }
                        accb = accb + cb;
                    }
                }
            }
        } else if (S.contrib_bf16) sum_contrib_slots<LPI, true, (LOCAL ? 4 : 8)>(S.contrib, S.cbias, b, e, pitch, L, k, acc, accb);
        else sum_contrib_slots<LPI, false, (LOCAL ? 4 : 8)>(S.contrib, S.cbias, b, e, pitch, L, k, acc, accb);
        if constexpr (LOCAL) {
            const long ti = t - S.nfb_rows, ts = ti - S.nitem_rows;
            const size_t row = t < S.nfb_rows ? (size_t)fb_off + (size_t)t
                             : ts < 0 ? (size_t)item_off + (size_t)ti : (size_t)user_off + S.shared_from + (size_t)ts;
            R c = io::load(W, row, pitch, L, k);
            add_rows(c, acc);
            io::store(W, row, pitch, L, k, c);
            if (L == 0 && (ts < 0 || S.user_bias)) bias[row] = bias[row] + accb;
        } else {
            wire_put<LPI, HALF>(dst, t, T, pitch, L, k, acc, accb);
        }
    }
    const long g0 = T * (long)(pitch + 1);
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < S.nglobal; g += (long)gridDim.x * blockDim.x) {
        const int b = S.gptr ? S.gptr[g] : 0, e = S.gptr ? S.gptr[g + 1] : 0;
        float acc = 0.0f;
        for (int s = b; s < e; s++) acc = acc + S.gcontrib[s];
        if (LOCAL) { if (b < e) g_bias[g] = g_bias[g] + acc; }
        else if (HALF) reinterpret_cast<__half *>(dst)[g0 + g] = __float2half_rn(acc);
        else reinterpret_cast<float *>(dst)[g0 + g] = acc;
    }
}

// ------------------------------------------------------------------------------------------------- kernel C: hot rows in ordered sub-steps
// One workgroup per hot row of the window, between the walk and the sums: the hot shared user rows (ITEM = false: S.hot[0 .. nhot); knob
// window_shared_sub; on user-group windows knob window_block_sub, section 6q: the FB build) in one launch, the hot item rows (ITEM = true: S.hot[nhot ..); knob window_item_sub, section 6m) in another.
// The row and its bias live in LDS; its slots are taken in file order, `sub` at a time.  One lane group per slot of a sub-step redoes the data row's
// update_inner the way k_wunit_walk does, statement for statement, with
//   * the hot row and its bias as the previous sub-step left them (LDS) -- at the hot entry's own position: in uent for a user row, in ent for a
//     plain item entry, in ient for a feature_item child (whose parent entry is read as of the window start, like every other row),
//   * the private user's row and bias as the walk held them when it reached the data row (the slot's record, written by the walk),
//   * everything else from the model, which is still as of the window start: a window with a hot row has no in-place single applies (the builder
//     gives every contribution a slot there), the sums run after this kernel, and this kernel does not write the model either -- another hot row of
//     the same data row (of either side) must read this one as of the window start, so the row's final value goes to its first slot and k_wunit_sum
//     moves it in;
// and parks new - current of the hot row (and bias) in LDS.  The parked changes of a sub-step are added in slot order (acc = +0 + c_1 + c_2 ...; every
// column by one thread) and the row moves by the sum.  The workgroup is sized to the sub-step: min(sub, 256 / LPI) lane groups; a larger sub-step
// takes several rounds of them (k = 64, sub = 128: 8 rounds of 16), the parked changes joining the sum round by round, in slot order all the same.
// FB (knob window_block_sub, section 6q; ITEM: knob window_block_item_sub, section 6u): the data rows belong to user-group spans -- tmp_ufactor starts from the span's tmp_ufeedback and
// calc_bias ends with tmp_ufeedback_bias, both as the walk held them when it reached the data row (the record's row of S.hfb / word of S.hfbb).
template <int LPI, bool ITEM, bool FB = false>
__global__ __launch_bounds__(256) void k_wunit_apply_hot(const DevParams P, const WUnitSchedule S) {
    extern __shared__ __align__(16) float hot_lds[];
    const int pitch = P.pitch, k = P.k, k4 = (k + 3) & ~3;
    const int G = blockDim.x / LPI, tid = threadIdx.x;
    const int g = tid / LPI, L = tid & (LPI - 1);
    float *cur = hot_lds;                    // [pitch] the row as the previous sub-step left it
    float *accv = cur + pitch;               // [pitch] the sub-step's sum so far
    float *park = accv + pitch;              // [G][pitch] the changes of the slots in flight
    float *pb = park + (size_t)G * pitch;    // [G] their bias changes
    float *sc = pb + G;                      // the bias as the previous sub-step left it, the sub-step's bias sum
    const WinHot h = S.hot[(ITEM ? S.nhot : 0) + blockIdx.x];
    const int sub = ITEM ? S.item_sub : S.hot_sub;
    const bool ub = P.no_user_bias == 0;
    const bool hbias = ITEM || ub;           // the item bias is always there
    const bool owns = !(LPI * 4 > k && L * 4 >= k);
    const float lr = P.lr;
    const size_t srow0 = (size_t)P.user_off + S.shared_from;
    const size_t hrow = ITEM ? (size_t)P.item_off + (size_t)h.j : srow0 + (size_t)h.j;
    const float wd_h = ITEM ? get_wd(P.i_rng, (unsigned)h.j, P.wd_item) : get_wd(P.u_rng, S.shared_from + (unsigned)h.j, P.wd_user);
    for (int c = tid; c < k4; c += blockDim.x) cur[c] = P.W[hrow * pitch + c];
    if (tid == 0) sc[0] = hbias ? P.bias[hrow] : 0.0f;
    __syncthreads();
    for (int s0 = h.b; s0 < h.e; s0 += sub) {
        const int s1 = min(s0 + sub, h.e);
        for (int c = tid; c < k4; c += blockDim.x) accv[c] = 0.0f;
        if (tid == 0) sc[1] = 0.0f;
        for (int q0 = s0; q0 < s1; q0 += G) {
            const int slot = q0 + g;
            if (slot < s1) {
                const int rix = h.rec + (slot - h.b);
                const WinHotRec rc = S.hrec[rix];
                const int r = rc.row;
                // where the hot entry sits: hu in uent (user side), he in ent or hc in ient (item side); -1: not there
                const int hu = ITEM ? -1 : rc.pos, he = (ITEM && rc.pos >= 0) ? rc.pos : -1, hc = (ITEM && rc.pos < 0) ? ~rc.pos : -1;
                int e0, e1, e2;
                if (S.rptr) { e0 = S.rptr[2 * (long)r]; e1 = S.rptr[2 * (long)r + 1]; e2 = S.rptr[2 * (long)r + 2]; }
                else { e0 = r * S.estride; e1 = e0 + S.estride - 1; e2 = e1 + 1; }
                const float label = S.label[r];
                const float ua = S.uval ? S.uval[r] : 1.0f;
                int u0 = 0, um = 0, u1 = 0;
                if (S.uptr) { u0 = S.uptr[r]; um = u0 + S.upos[r]; u1 = S.uptr[r + 1]; }
                int c0 = 0, c1 = 0;
                if (S.iptr) { c0 = S.iptr[r]; c1 = S.iptr[r + 1]; }
                const float4 p = load_row<LPI>(S.contrib, (size_t)slot, pitch, L, k);   // the walk's record
                const float bu = ub ? S.cbias[slot] : 0.0f;
                const float4 hw = owns ? *reinterpret_cast<const float4 *>(cur + L * 4) : f4zero();
                const float hb = sc[0];
                // ---- pred: k_wunit_walk's statements, the hot entry's row and bias from LDS
                double bs = 0.0;
                for (int j = e0; j < e1; j++) { const WinEnt e = S.ent[j]; bs += (double)(e.val * P.g_bias[e.idx]); }
                if (ub) {
                    for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * (j == hu ? hb : P.bias[srow0 + e.idx])); }
                    bs += (double)(ua * bu);
                    for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * (j == hu ? hb : P.bias[srow0 + e.idx])); }
                    bs += (double)(FB ? S.hfbb[rix] : 0.0f);
                }
                bs += 0.0;
                for (int j = e1, c = c0; j < e2; j++) {
                    const WinEnt e = S.ent[j];
                    bs += (double)(e.val * (j == he ? hb : P.bias[P.item_off + e.idx]));
                    for (; c < c1 && S.ient[c].pad == j; c++) { const WinEnt ch = S.ient[c]; bs += (double)((c == hc ? hb : P.bias[P.item_off + ch.idx]) * ch.val * e.val); }
                }
                double sum = (double)P.base_score + bs;
                float4 tu = FB ? load_row<LPI>(S.hfb, (size_t)rix, pitch, L, k) : f4zero();
                for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; axpy4(tu, j == hu ? hw : load_row<LPI>(P.W, srow0 + e.idx, pitch, L, k), e.val); }
                axpy4(tu, p, ua);
                for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; axpy4(tu, j == hu ? hw : load_row<LPI>(P.W, srow0 + e.idx, pitch, L, k), e.val); }
                float4 ti = f4zero();
                for (int j = e1, c = c0; j < e2; j++) {
                    const WinEnt e = S.ent[j];
                    axpy4(ti, j == he ? hw : load_row<LPI>(P.W, P.item_off + e.idx, pitch, L, k), e.val);
                    for (; c < c1 && S.ient[c].pad == j; c++) {
                        const WinEnt ch = S.ient[c];
                        axpy4(ti, c == hc ? hw : load_row<LPI>(P.W, P.item_off + ch.idx, pitch, L, k), (float)((double)ch.val * (double)e.val));
                    }
                }
                sum += (double)group_dot<LPI>(tu, ti, L, k);
                const float pred = map_active((float)sum, P.active_type);
                const float err = cal_grad(label, pred, P.active_type) * 1.0f;
                float4 ws = hw;
                float cb = 0.0f;
                if (ITEM) {
                    // ---- the hot row's part of update_no_decay + reg_item: the walk's item block (a plain entry: lr err ival; a child (c, v) of a parent
                    // with value ival: ((lr err) v) ival) against the current row
                    float si;
                    if (hc < 0) si = lr * err * S.ent[he].val;
                    else { const WinEnt ch = S.ient[hc]; si = lr * err * ch.val * S.ent[ch.pad].val; }
                    axpy4(ws, tu, si);
                    float nb = hb + si;
                    reg_row<LPI>(P, ws, wd_h, true, L);
                    nb = nb * (1.0f - lr * P.wd_item_bias);
                    sub4(ws, hw);
                    cb = nb - hb;
                } else {
                    // ---- the hot row's part of update_no_decay + reg_user: the walk's shared-row block against the current row
                    const float ss = lr * err * S.uent[hu].val;
                    axpy4(ws, ti, ss);
                    reg_row<LPI>(P, ws, wd_h, false, L);
                    sub4(ws, hw);
                    if (ub) { float nb = hb + ss; nb = nb * (1.0f - lr * P.wd_user_bias); cb = nb - hb; }
                }
                if (owns) *reinterpret_cast<float4 *>(park + (size_t)g * pitch + L * 4) = ws;
                if (L == 0) pb[g] = cb;
            }
            __syncthreads();
            const int m = min(G, s1 - q0);
            for (int c = tid; c < k4; c += blockDim.x) {
                float a = accv[c];
                for (int q = 0; q < m; q++) a = a + park[(size_t)q * pitch + c];
                accv[c] = a;
            }
            if (tid == 0) {
                float a = sc[1];
                for (int q = 0; q < m; q++) a = a + pb[q];
                sc[1] = a;
            }
            __syncthreads();
        }
        for (int c = tid; c < k4; c += blockDim.x) cur[c] = cur[c] + accv[c];
        if (tid == 0) sc[0] = sc[0] + sc[1];
        __syncthreads();
    }
    for (int c = tid; c < k4; c += blockDim.x) S.contrib[(size_t)h.b * pitch + c] = cur[c];
    if (tid == 0) S.cbias[h.b] = sc[0];
}

// the workgroup of a sub-step of `sub` slots: whole waves, min(sub, 256 / lpi) lane groups rounded up; LDS = current row, sum, G parked changes
template <bool ITEM, bool FB = false>
static void launch_wunit_apply_hot(const DevParams &P, const WUnitSchedule &S, long nrows, int sub, hipStream_t st) {
    if (nrows <= 0 || sub <= 0) return;
    const int lpi = lanes_per_instance(P.k);
    const long want = (long)std::min(sub, 256 / lpi) * lpi;
    const int block = (int)std::min<long>(256, (want + 63) / 64 * 64);
    const int G = block / lpi;
    const size_t lds = ((size_t)(2 + G) * (size_t)P.pitch + (size_t)G + 2) * sizeof(float);
    SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_apply_hot<LPI, ITEM, FB>), dim3((unsigned)nrows), dim3((unsigned)block), lds, st, P, S));
}
// feedback: the window's rows belong to user-group spans (window_block_sub; the walk left their feedback state in S.hfb / S.hfbb)
void launch_wunit_apply_shared(const DevParams &P, const WUnitSchedule &S, hipStream_t st, bool feedback) {
    if (feedback) launch_wunit_apply_hot<false, true>(P, S, S.nhot, S.hot_sub, st);
    else launch_wunit_apply_hot<false>(P, S, S.nhot, S.hot_sub, st);
}
// nitem_hot: the hot item rows of the window, S.hot[S.nhot .. S.nhot + nitem_hot)
void launch_wunit_apply_item(const DevParams &P, const WUnitSchedule &S, long nitem_hot, hipStream_t st, bool feedback) {
    if (feedback) launch_wunit_apply_hot<true, true>(P, S, nitem_hot, S.item_sub, st);   // user-group windows: knob window_block_item_sub
    else launch_wunit_apply_hot<true>(P, S, nitem_hot, S.item_sub, st);
}

// ------------------------------------------------------------------------------------------------- scoring (read-only)
// svdf_predict_dataset / svdf_eval_dataset on a window of user units.  Nothing is updated, so the rows are independent: they are scored
// LPI lanes per row, not walked unit by unit.  Three launches per window:
//   k_wunit_score_columns  the user and the segment of every regrouped row (one wave per unit spreads its segments' row ranges);
//   k_wunit_score_prepare  user-group trainers: prepare_ufeedback (apex_svd_base.h:523-538) once per segment, k_wunit_walk's prepare block in
//                          list order -- the sum of the feedback rows and of their biases, into a scratch row per segment;
//   k_wunit_score          the walk's pred block statement for statement (:445-454; SVDPPFeature::predict :583-591 for user-group rows), the user's
//                          row and bias from the model as it stands.
// Every layout variant of a window is read -- estride / rptr rows, uval absent, the shared user section, the feature_item child section -- and of
// an entry only idx, val and (children) pad = the parent's position: slots and the hot lanes' marks (ent.pad, uent.pad, child slots <= -2) are
// not looked at.  A score equals svdf_predict_csr_batch's / svdf_predict_block's for the same row bit for bit.
__global__ __launch_bounds__(256) void k_wunit_score_columns(const WUnitSchedule S, unsigned *user_col, int *seg_col) {
    const int lane = threadIdx.x & 63;
    const long uidx = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (uidx >= S.nunits) return;
    const WinUnit un = S.units[uidx];
    for (int sg = 0; sg < un.seg_count; sg++) {
        const WinSeg seg = sg == 0 ? un.first : S.segs[un.seg_begin + sg];
        for (int j = lane; j < seg.row_count; j += 64) {
            user_col[seg.row_begin + j] = un.user;
            seg_col[seg.row_begin + j] = un.seg_begin + sg;
        }
    }
}
template <int LPI, typename R = float4>
__global__ __launch_bounds__(256) void k_wunit_score_prepare(const DevParams P, const WUnitSchedule S, long nseg, float *fbvec, float *fbbias) {
    using io = row_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63;
    const int L = lane & (LPI - 1);
    const long q = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW + lane / LPI;
    if (q >= nseg) return;
    const WinSeg seg = S.segs[q];
    const int pitch = P.pitch, k = P.k;
    const bool ub = P.no_user_bias == 0;
    R tmp_fb = row_traits<R>::zero();
    float tmp_bias = 0.0f;
    for (int j = seg.fb_begin; j < seg.fb_begin + seg.fb_count; j++) {
        const WinEnt f = S.fbent[j];
        const unsigned row = P.fb_off + f.idx;
        axpy4(tmp_fb, io::load(P.W, row, pitch, L, k), f.val);
        if (ub) tmp_bias = tmp_bias + P.bias[row] * f.val;
    }
    io::store(fbvec, (size_t)q, pitch, L, k, tmp_fb);   // (slot by slot for a wide row)
    if (L == 0) fbbias[q] = tmp_bias;
}
template <int LPI, bool FB, typename R = float4>
__global__ __launch_bounds__(256) void k_wunit_score(const DevParams P, const WUnitSchedule S, const unsigned *user_col, const int *seg_col,
                                                     const float *fbvec, const float *fbbias, long nrow, const int *pos, float *out) {
    using io = row_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63;
    const int L = lane & (LPI - 1);
    const long gidx = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW + lane / LPI;
    const long stride = (long)gridDim.x * (blockDim.x >> 6) * IPW;
    const int pitch = P.pitch, k = P.k;
    const bool ub = P.no_user_bias == 0;
    const size_t srow0 = (size_t)P.user_off + S.shared_from;
    for (long r = gidx; r < nrow; r += stride) {
        const unsigned ur = P.user_off + user_col[r];
        const R p = io::load(P.W, ur, pitch, L, k);
        const float bu = ub ? P.bias[ur] : 0.0f;
        R tmp_fb = row_traits<R>::zero();
        float tmp_bias = 0.0f;
        if (FB) {
            const int q = seg_col[r];
            tmp_fb = io::load(fbvec, (size_t)q, pitch, L, k);
            tmp_bias = fbbias[q];
        }
        int e0, e1, e2;
        if (S.rptr) { e0 = S.rptr[2 * r]; e1 = S.rptr[2 * r + 1]; e2 = S.rptr[2 * r + 2]; }
        else { e0 = (int)r * S.estride; e1 = e0 + S.estride - 1; e2 = e1 + 1; }
        const float ua = S.uval ? S.uval[r] : 1.0f;
        int u0 = 0, um = 0, u1 = 0;
        if (S.uptr) { u0 = S.uptr[r]; um = u0 + S.upos[r]; u1 = S.uptr[r + 1]; }
        int c0 = 0, c1 = 0;
        if (S.iptr) { c0 = S.iptr[r]; c1 = S.iptr[r + 1]; }
        // ---- pred: k_wunit_walk's statements
        double bs = 0.0;
        for (int j = e0; j < e1; j++) { const WinEnt e = S.ent[j]; bs += (double)(e.val * P.g_bias[e.idx]); }
        if (ub) {
            for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * P.bias[srow0 + e.idx]); }
            bs += (double)(ua * bu);
            for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; bs += (double)(e.val * P.bias[srow0 + e.idx]); }
            bs += (double)(FB ? tmp_bias : 0.0f);
        }
        bs += 0.0;
        for (int j = e1, c = c0; j < e2; j++) {
            const WinEnt e = S.ent[j];
            bs += (double)(e.val * P.bias[P.item_off + e.idx]);
            for (; c < c1 && S.ient[c].pad == j; c++) { const WinEnt ch = S.ient[c]; bs += (double)(P.bias[P.item_off + ch.idx] * ch.val * e.val); }
        }
        double sum = (double)P.base_score + bs;
        R tu = FB ? tmp_fb : row_traits<R>::zero();
        for (int j = u0; j < um; j++) { const WinEnt e = S.uent[j]; axpy4(tu, io::load(P.W, srow0 + e.idx, pitch, L, k), e.val); }
        axpy4(tu, p, ua);
        for (int j = um; j < u1; j++) { const WinEnt e = S.uent[j]; axpy4(tu, io::load(P.W, srow0 + e.idx, pitch, L, k), e.val); }
        R ti = row_traits<R>::zero();
        for (int j = e1, c = c0; j < e2; j++) {
            const WinEnt e = S.ent[j];
            axpy4(ti, io::load(P.W, P.item_off + e.idx, pitch, L, k), e.val);
            for (; c < c1 && S.ient[c].pad == j; c++) {
                const WinEnt ch = S.ient[c];
                axpy4(ti, io::load(P.W, P.item_off + ch.idx, pitch, L, k), (float)((double)ch.val * (double)e.val));
            }
        }
        sum += (double)group_dot<LPI>(tu, ti, L, k);
        if (L == 0) out[pos ? (long)pos[r] : r] = map_active((float)sum, P.active_type);
    }
}
void launch_wunit_score_columns(const WUnitSchedule &S, unsigned *user_col, int *seg_col, hipStream_t st) {
    if (S.nunits <= 0) return;
    const long blocks = (S.nunits * 64 + 255) / 256;
    hipLaunchKernelGGL(k_wunit_score_columns, dim3((unsigned)blocks), dim3(256), 0, st, S, user_col, seg_col);
}
void launch_wunit_score_prepare(const DevParams &P, const WUnitSchedule &S, long nseg, float *fbvec, float *fbbias, hipStream_t st) {
    if (nseg <= 0) return;
    const int lpi = lanes_per_instance(P.k);
    const long per_block = 4L * (64 / lpi);
    const long grid = (nseg + per_block - 1) / per_block;
    SVDF_DISPATCH_ROW(P.k, hipLaunchKernelGGL((k_wunit_score_prepare<LPI, R>), dim3((unsigned)grid), dim3(256), 0, st, P, S, nseg, fbvec, fbbias));   // (wide rows: a wave per segment)
}
void launch_wunit_score(const DevParams &P, const WUnitSchedule &S, bool feedback, const unsigned *user_col, const int *seg_col, const float *fbvec,
                        const float *fbbias, long nrow, const int *pos, float *out, hipStream_t st) {
    if (nrow <= 0) return;
    const int lpi = lanes_per_instance(P.k);
    const int grid = grid_for(nrow, lpi, 256 * 8);
    if (feedback) { SVDF_DISPATCH_ROW(P.k, hipLaunchKernelGGL((k_wunit_score<LPI, true, R>), dim3(grid), dim3(256), 0, st, P, S, user_col, seg_col, fbvec, fbbias, nrow, pos, out)); }
    else { SVDF_DISPATCH_ROW(P.k, hipLaunchKernelGGL((k_wunit_score<LPI, false, R>), dim3(grid), dim3(256), 0, st, P, S, user_col, seg_col, fbvec, fbbias, nrow, pos, out)); }
}

bool wunit_fast_applies(const DevParams &P, const WUnitSchedule &S, bool feedback) {
    if (!(P.k == 64 || P.k == 128) || S.rptr != nullptr || S.uval != nullptr || P.reg_method == 2) return false;
    const int ng = S.estride - 1;
    return ng == 0 || (ng == 4 && !feedback);
}
int launch_wunit_walk(const DevParams &P, const WUnitSchedule &S, bool feedback, int fast, hipStream_t st, bool shared_uniform) {
    if (S.nunits <= 0) return 0;
    // user-group windows whose segments carry one user section each (shared_uniform, the builder's flag): the wave form that holds
    // the section's rows in registers, under the plain wave form's conditions.  Opt-in (fast = 3) until it has been measured against the general walk on
    // an MI355X (profiles/r15_block_shared.md); fast = 3 is fast = 2 otherwise
    if (fast >= 3 && S.uptr && shared_uniform && !S.iptr && !S.hot && !S.contrib_bf16 && wunit_wave_applies(P, S, feedback) && S.nunits <= 16384) {
        launch_wunit_wave(P, S, st, true);
        return 1;
    }
    if (S.uptr || S.iptr || S.hot) fast = 0;   // rows with shared user entries or feature_item children, windows with hot rows (the records of the ordered sub-steps): the general walk
    // fast: 0 = the general lane-group kernel, 1 = the slot kernel where it applies, 2 (default) = in addition one WAVE per unit for user-group
    // windows whose launch does not fill the chip anyway (its time is the longest unit's latency: svdf_k_wave.hip, k_wunit_wave)
    if (fast >= 2 && wunit_wave_applies(P, S, feedback) && S.nunits <= 16384) { launch_wunit_wave(P, S, st); return 2; }
    if (fast && wunit_fast_applies(P, S, feedback)) {
        auto go = [&](auto lanes) {
            constexpr int LANES = decltype(lanes)::value;
            const long per_wave = 64 / LANES;
            const long waves = (S.nunits + per_wave - 1) / per_wave;
            if (S.estride == 1) {
                if (feedback) hipLaunchKernelGGL((k_wunit_fast<LANES, 2, true, 0, 4>), dim3((unsigned)waves), dim3(64), 0, st, P, S);
                else hipLaunchKernelGGL((k_wunit_fast<LANES, 2, false, 0, 4>), dim3((unsigned)waves), dim3(64), 0, st, P, S);
            } else {
                hipLaunchKernelGGL((k_wunit_fast<LANES, 2, false, 4, 1>), dim3((unsigned)waves), dim3(64), 0, st, P, S);
            }
        };
        if (P.k == 64) go(std::integral_constant<int, 8>());
        else go(std::integral_constant<int, 16>());
        return 0;
    }
    const int lpi = lanes_per_instance(P.k);
    const long ipw = 64 / lpi;
    const long waves = (S.nunits + ipw - 1) / ipw;
    if (P.k > 256) {   // wide rows: the general walk, one wave per unit; no fast, slot or wave form (the predicates above say no), no hot rows
                       // (the sub-step lanes keep one lane group per slot: the host refuses their knobs at these widths)
        if (S.hot) throw std::runtime_error("k_wunit_walk: ordered sub-steps need num_factor <= 256");
        if (feedback) { SVDF_DISPATCH_WIDE(P.k, hipLaunchKernelGGL((k_wunit_walk<LPI, true, false, R>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
        else { SVDF_DISPATCH_WIDE(P.k, hipLaunchKernelGGL((k_wunit_walk<LPI, false, false, R>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
        return 0;
    }
    if (feedback && S.hot) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_walk<LPI, true, true>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
    else if (feedback) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_walk<LPI, true>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
    else if (S.hot) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_walk<LPI, false, true>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
    else { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_walk<LPI, false>), dim3((unsigned)waves), dim3(64), 0, st, P, S)); }
    return 0;
}
// dst == nullptr: add the sums to the model in place; else the wire buffer (half: fp16)
void launch_wunit_sum(const DevParams &P, const WUnitSchedule &S, void *dst, int half, hipStream_t st) {
    const long T = S.nfb_rows + S.nitem_rows + (dst ? 0 : S.nshared_rows);
    if (T <= 0 && S.nglobal <= 0) return;
    const int lpi = lanes_per_instance(P.k);
    const long ipw = 64 / lpi;
    const long work = (!dst && S.touched) ? S.ntouched : T;   // in place over the list of targets with slots, else every target
    long waves = (std::max<long>(work, 1) + ipw - 1) / ipw;
    long grid = (waves + 3) / 4;
    // (many short-lived waves beat one resident set walking several targets each: grid cap 2 048 -> 53.5 us, 4 096 -> 45.8, 16 384 -> 43.8 per SVD++ window)
    if (grid > 16384) grid = 16384;
    if (grid < 1) grid = 1;
    if (P.k > 256) {   // wide rows: the in-place sums of the one-GPU sequence, a wave per target (the N-rank builders stay at 256 factors: no wire buffer of wide rows)
        if (dst || S.hot) throw std::runtime_error("k_wunit_sum: the wire buffer and ordered sub-steps need num_factor <= 256");
        SVDF_DISPATCH_WIDE(P.k, hipLaunchKernelGGL((k_wunit_sum<LPI, false, true, false, R>), dim3((unsigned)grid), dim3(256), 0, st, S, P.W, P.bias, P.g_bias, P.fb_off, P.item_off, P.user_off, P.pitch, P.k, (void *)nullptr));
        return;
    }
    if (!dst && S.hot) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_sum<LPI, false, true, true>), dim3((unsigned)grid), dim3(256), 0, st, S, P.W, P.bias, P.g_bias, P.fb_off, P.item_off, P.user_off, P.pitch, P.k, (void *)nullptr)); }
    else if (!dst) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_sum<LPI, false, true>), dim3((unsigned)grid), dim3(256), 0, st, S, P.W, P.bias, P.g_bias, P.fb_off, P.item_off, P.user_off, P.pitch, P.k, (void *)nullptr)); }
    else if (half) { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_sum<LPI, true, false>), dim3((unsigned)grid), dim3(256), 0, st, S, P.W, P.bias, P.g_bias, P.fb_off, P.item_off, P.user_off, P.pitch, P.k, dst)); }
    else { SVDF_DISPATCH_LPI(lpi, hipLaunchKernelGGL((k_wunit_sum<LPI, false, false>), dim3((unsigned)grid), dim3(256), 0, st, S, P.W, P.bias, P.g_bias, P.fb_off, P.item_off, P.user_off, P.pitch, P.k, dst)); }
}

}  // namespace svdf

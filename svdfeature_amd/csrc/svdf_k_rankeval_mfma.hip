// svdf_k_rankeval_mfma.hip -- rank positions through a certified counting sweep on the matrix cores (knob rank_eval_prefilter = 1,
// DESIGN.md section 6aj): what k_rank_eval_sweep counts, count for count, wherever the rule of include/svdfeature_amd.h certifies a section.
//
// A position is an integer count against a threshold, the pinned score p_t of positive t (k_rank_eval_pos, unchanged).  The approximate
// score a of a candidate -- the matrix sweep's, section 6ah -- lies within Delta_s of its pinned score (section 6ai), so a > hi_t =
// up(p_t + Delta_s) says the pinned score is greater than p_t, a < lo_t = down(p_t - Delta_s) that it is smaller, and only the candidates
// in the band between the two need the pinned chain.  Three kernels behind k_rank_eval_pos:
//
// k_rank_eval_prep, one wave per section: H_s, Delta_s and the checks on the section's row u in float64 (k_rank_topn_exact's statement, the
// same envelope), then the section's positives in ascending order of (pinned score, id) -- each lane ranks its positives by counting, so the
// order is a function of the keys alone -- and lo / hi per positive in that order.  Because Delta_s is shared, lo and hi are sorted alike.
//
// k_rank_eval_sweep_mfma, the counting sweep.  The score is k_rank_topn_sweep_mfma's: both kernels call mx_sweep (svdf_k_rankmfma.h), which
// states the tiling, the K map, the stage, the ban masks one tile ahead, the bias add and the output layout once.  A ROW is a section or a
// slice of at most RANK_EVAL_MX_POS of its sorted positives.  The workgroup keeps its rows' lo / hi and a histogram
// [64][RANK_EVAL_MX_POS + 1] in LDS for its whole item range.  Per live score, in the MFMA's own output layout: ONE compare against the
// row's lo_0 -- the common case ends there.  Otherwise the wave walks its rows that have such scores: j = the number of the row's positives
// with hi_t < a; the candidate is in the band iff j < T and a >= lo_j, else hist[row][j] += 1 (an LDS integer atomic) when j > 0.  A row's
// band candidates of a tile are appended to its list in HBM by ballot prefix behind one integer atomic on the row's cursor, which keeps
// counting past the capacity; ids beyond it are not stored.  At the end of the range positive t receives the sum of hist[row][j] over
// j > t into `greater`.
//
// k_rank_eval_band, one wave per row: u once into LDS, the row's band ids re-scored 64 at a time in the pinned order (tx_pinned_scores,
// svdf_k_rankgather.h) and compared with every positive of the row by k_rank_eval_sweep's rule (greater / tied / tied with a smaller id,
// +0 == -0, a positive is not its own candidate); integer atomics; one `certified` word per row.  Banned candidates never enter a count, so
// k_rank_eval_ban has nothing to take back.
#include <cstdlib>

#include "svdf_k_rankgather.h"
#include "svdf_k_rankmfma.h"

namespace svdf {

constexpr int EM_POS = RANK_EVAL_MX_POS;  // positives of a row
constexpr unsigned EM_ABS = 0x7fffffffu, EM_INF = 0x7f800000u, EM_MIN_NORMAL = 0x00800000u, EM_NAN = 0x7fc00000u;

// bit 0: |x| is inf or NaN; bit 1: denormal -- on the bit pattern of |x| (ev_flags of svdf_k_ranktopn_exact.hip)
__device__ __forceinline__ unsigned em_flags(unsigned ab) { return (ab >= EM_INF ? 1u : 0u) | (ab - 1u < EM_MIN_NORMAL - 1u ? 2u : 0u); }

// the float next to f towards -inf / +inf (f finite or an infinity that the direction leaves)
__device__ __forceinline__ float em_step(float f, bool up) {
    const unsigned b = __float_as_uint(f);
    if ((b & EM_ABS) == 0u) return __uint_as_float(up ? 1u : 0x80000001u);
    return __uint_as_float(((b >> 31) != 0u) == up ? b - 1u : b + 1u);
}
// float32(d) rounded down / up: the nearest float, moved one step where it lies on the wrong side of d
__device__ __forceinline__ float em_round(double d, bool up) {
    const float f = (float)d;
    if (up ? (double)f < d : (double)f > d) return em_step(f, up);
    return f;
}

__global__ __launch_bounds__(64) void k_rank_eval_prep(const DevParams P, const RankEvalMxDev D) {
    const int sec = blockIdx.x, lane = threadIdx.x;
    const int q0 = D.sec_p0[sec], q1 = D.sec_p0[sec + 1];
    if (q0 == q1) return;   // a section without positives has no rows
    const int k = P.k, nq = P.pitch >> 2;
    // ---- H_s and (a) for u in float64, Delta_s: k_rank_topn_exact's statement
    const float4 *urow = re_section_row(P, D.user_rows, D.sec_user, sec);
    double h = 0.0;
    unsigned uflags = 0u;
    for (int q = lane; q < nq; q += 64) {
        const float4 u = urow[q];
        const float ue[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (4 * q + e < k) {
                const unsigned ab = __float_as_uint(ue[e]) & EM_ABS;
                uflags |= em_flags(ab);
                h += (double)__uint_as_float(ab) * (double)__uint_as_float(D.envelope[4 * q + e]);
            }
    }
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
    const double H = (double)__uint_as_float(D.envelope[RANK_ENV_BIAS]) + h;
    const double delta = 4.0 * (double)(k + 2) * 0x1p-24 * H + (double)(k + 2) * 0x1p-124;
    // (a), (b); a NaN or inf in H fails the comparison
    const bool ok = D.envelope[RANK_ENV_FLAGS] == 0u && __ballot(uflags != 0u) == 0ull && H <= 0x1p126;
    // ---- the positives in ascending (score word, ~id): the rank of one is the number of smaller keys, whoever counts them.  T^2 key reads
    // from L2 for a section of T positives: nothing at the hundreds a section brings, seconds at tens of thousands
    bool pnan = false;
    const float none = __uint_as_float(EM_NAN);
    for (int i = q0 + lane; i < q1; i += 64) {
        const float p = D.pos_score[i];
        const tn_key_t key = tn_key(p, D.pos_item[i]);
        int rank = 0;
        for (int j = q0; j < q1; j++) rank += tn_key(D.pos_score[j], D.pos_item[j]) < key ? 1 : 0;
        pnan = pnan || p != p;
        D.srt[q0 + rank] = i;
        // a section that fails (a) or (b) is ranked again whatever the sweep counts: NaN thresholds, which no compare passes (a +inf score
        // included), keep its candidates off the slow path
        D.lo[q0 + rank] = ok ? em_round((double)p - delta, false) : none;
        D.hi[q0 + rank] = ok ? em_round((double)p + delta, true) : none;
    }
    const bool clean = __ballot(pnan) == 0ull;   // a NaN among the positives' own scores: the pinned route flags the section
    if (lane == 0) D.sec_ok[sec] = ok && clean ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_rank_eval_sweep_mfma(const DevParams P, const RankEvalMxDev D) {
    __shared__ MxLds L;
    __shared__ float l_lo[MX_TS][EM_POS], l_hi[MX_TS][EM_POS];
    __shared__ int l_hist[MX_TS][EM_POS + 1];
    __shared__ int l_T[MX_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;
    const int row_base = blockIdx.x * MX_TS;
    const int nrows = D.nrow - row_base < MX_TS ? D.nrow - row_base : MX_TS;
    // the rows' thresholds, for the whole item range; a row past the last has none, and a lo_0 that no compare passes
    // (all of this is read behind mx_sweep's first barrier)
    for (int q = tid; q < MX_TS * EM_POS; q += 256) {
        const int row = q / EM_POS, t = q - row * EM_POS;
        float lo = __uint_as_float(EM_NAN), hi = lo;
        if (row < nrows) {
            const int p0 = D.row_p0[row_base + row], T = D.row_p0[row_base + row + 1] - p0;
            if (t < T) { lo = D.lo[p0 + t]; hi = D.hi[p0 + t]; }
        }
        l_lo[row][t] = lo; l_hi[row][t] = hi;
    }
    for (int q = tid; q < MX_TS * (EM_POS + 1); q += 256) (&l_hist[0][0])[q] = 0;
    for (int q = tid; q < MX_TS; q += 256) l_T[q] = q < nrows ? D.row_p0[row_base + q + 1] - D.row_p0[row_base + q] : 0;

    mx_sweep(P, D.user_rows, D.sec_user, D.item_rows, D.item_bias, D.ban_p0, D.ban_item, D.items_per_block, nrows, L,
             [&](int row) { return D.row_sec[row_base + row]; },
             [&](long it0, int row0, const mx_f4 *acc, unsigned live) {
        unsigned slow = 0u;   // bit 4 b + r: not certainly below every positive of its row
        float lo0[4];
#pragma unroll
        for (int r = 0; r < 4; r++) lo0[r] = l_lo[row0 + r][0];
#pragma unroll
        for (int b = 0; b < MX_NB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (((live >> (4 * b + r)) & 1u) && acc[b][r] >= lo0[r]) slow |= 1u << (4 * b + r);
        if (!__ballot(slow != 0u)) return;   // the common case: one compare per score
        const tn_key_t below = (1ull << lane) - 1ull;
        for (int gq = 0; gq < 4; gq++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned bits = lgrp == gq ? (slow >> r) & 0x11111111u : 0u;   // bit 4 b: the 16 lanes that hold this row
                if (!__ballot(bits != 0u)) continue;   // wave-uniform
                const int row = wave * 16 + 4 * gq + r, T = l_T[row];
                const float *lo = l_lo[row], *hi = l_hi[row];
                unsigned band = 0u;   // bit b
#pragma unroll
                for (int b = 0; b < MX_NB; b++)
                    if ((bits >> (4 * b)) & 1u) {
                        const float a = acc[b][r];
                        int j = 0;
                        while (j < T && hi[j] < a) j++;   // the positives this candidate certainly beats
                        if (j < T && a >= lo[j]) band |= 1u << b;
                        else if (j > 0) atomicAdd(&l_hist[row][j], 1);
                    }
                // the band candidates of the row in this tile: one atomic on its cursor, places by ballot prefix
                int n = 0;
#pragma unroll
                for (int b = 0; b < MX_NB; b++) n += __popcll(__ballot((band >> b) & 1u));
                if (n == 0) continue;   // wave-uniform
                int at = 0;
                if (lane == 0) at = atomicAdd(&D.band_cursor[row_base + row], n);   // keeps counting past the capacity
                at = __builtin_amdgcn_readfirstlane(at);
                int *list = D.band_list + (size_t)(row_base + row) * D.band_cap;
#pragma unroll
                for (int b = 0; b < MX_NB; b++) {
                    const bool take = (band >> b) & 1u;
                    const tn_key_t bl = __ballot(take);
                    const int mine = at + __popcll(bl & below);
                    if (take && mine < D.band_cap) list[mine] = (int)(it0 + 16 * b + lcol);   // ids beyond the capacity are not stored
                    at += __popcll(bl);
                }
            }
        }
    });
    // ---- positive t of a row is beaten by every candidate counted under a bucket j > t
    for (int q = tid; q < nrows; q += 256) {
        const int p0 = D.row_p0[row_base + q], T = l_T[q];
        int above = 0;
        for (int j = T; j >= 1; j--) {
            above += l_hist[q][j];
            if (above) atomicAdd(&D.greater[D.srt[p0 + j - 1]], above);
        }
        if (L.nan[q] && D.row_first[row_base + q]) atomicAdd(&D.nan_cnt[D.row_sec[row_base + q]], L.nan[q]);
    }
}


__global__ __launch_bounds__(64) void k_rank_eval_band(const DevParams P, const RankEvalMxDev D) {
    __shared__ float4 l_rows[64 * TX_LP];
    __shared__ float4 l_u[256];
    const int row = blockIdx.x, lane = threadIdx.x, sec = D.row_sec[row];
    const int total = D.band_cursor[row];
    // (a), (b) from k_rank_eval_prep, (c) from the sweep, (d) from the cursor: the section is ranked again, nothing here would be read
    if (!D.sec_ok[sec] || D.nan_cnt[sec] != 0 || total > D.band_cap) {
        if (lane == 0) D.row_cert[row] = 0;
        return;
    }
    const int nq = P.pitch >> 2;
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    const float4 *urow = re_section_row(P, D.user_rows, D.sec_user, sec);
    for (int q = lane; q < nq; q += 64) l_u[q] = urow[q];
    tn_wave_sync();
    const int *list = D.band_list + (size_t)row * D.band_cap;
    const int p0 = D.row_p0[row], p1 = D.row_p0[row + 1];
    bool pnan = false;
    for (int r0 = 0; r0 < total; r0 += 64) {
        bool on;
        int id;
        const float s = tx_pinned_scores(P, ibase, ibias, l_u, l_rows, r0, total, lane, [&](int i) { return list[i]; }, on, id);
        pnan = pnan || (on && s != s);
        for (int i = p0; i < p1; i++) {
            const int q = D.srt[i];
            const float t = D.pos_score[q];
            const int p = D.pos_item[q];
            const bool gt = on && s > t;
            const bool eq = on && s == t && id != p;   // +0 == -0, NaN equals nothing
            const int ngt = __popcll(__ballot(gt)), neq = __popcll(__ballot(eq)), nbf = __popcll(__ballot(eq && id < p));
            if (lane == 0) {
                if (ngt) atomicAdd(&D.greater[q], ngt);
                if (neq) atomicAdd(&D.tied[q], neq);
                if (nbf) atomicAdd(&D.before[q], nbf);
            }
        }
    }
    const bool clean = __ballot(pnan) == 0ull;   // a pinned NaN the matrix sweep did not see: the pinned route flags the section
    if (lane == 0) D.row_cert[row] = clean ? 1 : 0;
}

void launch_rank_eval_mx(const DevParams &P, const RankEvalMxDev &D, hipStream_t st) {
    if (D.npos <= 0 || D.nrow <= 0) return;
    // l_u holds 256 float4s, the envelope 1024 columns; a list shorter than a row's own positives would certify nothing
    if ((P.pitch >> 2) > 256 || P.k > 1024 || D.band_cap < 64 || D.gy < 1 || D.items_per_block < 1 || !D.envelope) abort();
    launch_rank_eval_pos(P, D, st);
    hipLaunchKernelGGL(k_rank_eval_prep, dim3((unsigned)D.nsec), dim3(64), 0, st, P, D);
    hipLaunchKernelGGL(k_rank_eval_sweep_mfma, dim3((unsigned)((D.nrow + MX_TS - 1) / MX_TS), (unsigned)D.gy), dim3(256), 0, st, P, D);
    hipLaunchKernelGGL(k_rank_eval_band, dim3((unsigned)D.nrow), dim3(64), 0, st, P, D);
}

}  // namespace svdf

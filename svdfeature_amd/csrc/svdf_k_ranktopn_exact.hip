// svdf_k_ranktopn_exact.hip -- the certified prefilter of the top-N calls (knob rank_topn_prefilter = 1): the pinned
// lists, bit for bit, behind the selecting sweep on the matrix cores (svdf_k_ranktopn_mfma.hip, section 6ah).
//
// The matrix sweep is launched unchanged and keeps M = top_n + slack keys per list.  Its contract puts every approximate score within
// Delta_s = 4 (k + 2) 2^-24 H_s + (k + 2) 2^-124 of the pinned score, H_s = B + sum_j |u_j| m_j, m_j = max_i |v_ij|, B = max_i |b_i| -- as
// long as every input is finite and zero or normal and H_s <= 2^126 (include/svdfeature_amd.h states the rule).  Two kernels:
//
// k_rank_item_envelope, once per call: m, B and the flags of the item side the sweep reads.  Item ranges across workgroups; inside a
// workgroup a lane owns float4 column quads and the waves stride over rows; rows of fewer than 64 float4s lie side by side in one wave
// (64 / nq rows), so a wave's load is one contiguous run of up to 1 KiB.  Maxima are taken on the bit patterns of the absolute values
// (an order-free integer maximum, NaN above inf above every number), per workgroup in LDS, between workgroups by atomicMax.
//
// k_rank_topn_exact, one wave per section, in the merge's place: merges the section's gy lists to the M largest approximate keys, reads
// the section's row u once (H_s and the checks on u, float64, one wave reduction), re-scores the at most M listed ids in the pinned order
// and certifies the section or leaves it to the pinned sweep.  The re-scoring walks the candidates 64 at a time and K in chunks of 64
// floats through LDS: tx_pinned_scores (svdf_k_rankgather.h), which the band pass of the counting sweep shares (section 6aj).
#include <algorithm>
#include <cstdlib>

#include "svdf_kernels.h"
#include "svdf_k_rankgather.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

constexpr int EV_UNROLL = 4;           // rows a lane has in flight
constexpr int EV_MAX_WG = 1024;        // workgroups of the envelope at the most
constexpr unsigned EV_ABS = 0x7fffffffu, EV_INF = 0x7f800000u, EV_MIN_NORMAL = 0x00800000u;

// bit 0: |x| is inf or NaN; bit 1: denormal -- on the bit pattern of |x|
__device__ __forceinline__ unsigned ev_flags(unsigned ab) { return (ab >= EV_INF ? 1u : 0u) | (ab - 1u < EV_MIN_NORMAL - 1u ? 2u : 0u); }

// QL: float4 quads of a row that one lane owns (rows of up to 64 QL float4s)
template <int QL>
__global__ __launch_bounds__(256) void k_rank_item_envelope(const DevParams P, const float *item_rows, const float *item_bias, unsigned *env) {
    __shared__ unsigned l_m[256 * QL];
    __shared__ unsigned l_b, l_f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = P.k, nq = P.pitch >> 2;
    const float *ibase = re_item_base(P, item_rows), *ibias = re_item_bias(P, item_bias);
    for (int j = tid; j < 256 * QL; j += 256) l_m[j] = 0u;
    if (tid == 0) { l_b = 0u; l_f = 0u; }
    __syncthreads();
    const long per = ((long)P.num_item + gridDim.x - 1) / gridDim.x;
    const long i0 = (long)blockIdx.x * per, i1 = i0 + per < (long)P.num_item ? i0 + per : (long)P.num_item;
    const int side = QL == 1 ? 64 / nq : 1;           // rows side by side in one wave
    const int sub = QL == 1 ? lane / nq : 0, q0 = QL == 1 ? lane - sub * nq : lane;
    uint4 keep[QL], mx[QL];                            // pads (k .. pitch) and quads past the row are masked out of everything
#pragma unroll
    for (int c = 0; c < QL; c++) {
        const int e = 4 * (q0 + 64 * c);
        keep[c] = make_uint4(e < k ? EV_ABS : 0u, e + 1 < k ? EV_ABS : 0u, e + 2 < k ? EV_ABS : 0u, e + 3 < k ? EV_ABS : 0u);
        mx[c] = make_uint4(0u, 0u, 0u, 0u);
    }
    unsigned flags = 0u;
    if (sub < side)
        for (long i = i0 + wave * side + sub; i < i1; i += 4 * side * EV_UNROLL) {
            uint4 v[EV_UNROLL][QL];
#pragma unroll
            for (int r = 0; r < EV_UNROLL; r++) {
                const long row = i + 4 * side * r;
#pragma unroll
                for (int c = 0; c < QL; c++) {
                    v[r][c] = make_uint4(0u, 0u, 0u, 0u);
                    if (row < i1 && q0 + 64 * c < nq) v[r][c] = reinterpret_cast<const uint4 *>(ibase + (size_t)row * P.pitch)[q0 + 64 * c];
                }
            }
#pragma unroll
            for (int r = 0; r < EV_UNROLL; r++)
#pragma unroll
                for (int c = 0; c < QL; c++) {
                    const uint4 a = make_uint4(v[r][c].x & keep[c].x, v[r][c].y & keep[c].y, v[r][c].z & keep[c].z, v[r][c].w & keep[c].w);
                    mx[c].x = a.x > mx[c].x ? a.x : mx[c].x; mx[c].y = a.y > mx[c].y ? a.y : mx[c].y;
                    mx[c].z = a.z > mx[c].z ? a.z : mx[c].z; mx[c].w = a.w > mx[c].w ? a.w : mx[c].w;
                    flags |= ev_flags(a.x) | ev_flags(a.y) | ev_flags(a.z) | ev_flags(a.w);
                }
        }
    unsigned bmax = 0u;
    for (long i = i0 + tid; i < i1; i += 256) {
        const unsigned ab = __float_as_uint(ibias[i]) & EV_ABS;
        bmax = ab > bmax ? ab : bmax;
        flags |= ev_flags(ab);
    }
    // ---- the workgroup's maxima in LDS, then one atomicMax per column that saw a non-zero
#pragma unroll
    for (int c = 0; c < QL; c++) {
        const int e = 4 * (q0 + 64 * c);
        if (mx[c].x) atomicMax(&l_m[e], mx[c].x);
        if (mx[c].y) atomicMax(&l_m[e + 1], mx[c].y);
        if (mx[c].z) atomicMax(&l_m[e + 2], mx[c].z);
        if (mx[c].w) atomicMax(&l_m[e + 3], mx[c].w);
    }
    if (bmax) atomicMax(&l_b, bmax);
    if (flags) atomicOr(&l_f, flags);
    __syncthreads();
    for (int j = tid; j < k; j += 256)
        if (l_m[j]) atomicMax(&env[j], l_m[j]);
    if (tid == 0) {
        if (l_b) atomicMax(&env[RANK_ENV_BIAS], l_b);
        if (l_f) atomicOr(&env[RANK_ENV_FLAGS], l_f);
    }
}

void launch_rank_item_envelope(const DevParams &P, const float *item_rows, const float *item_bias, unsigned *envelope, hipStream_t st) {
    const int nq = P.pitch >> 2;
    if (P.num_item <= 0 || nq < 1 || nq > 256 || P.k > 4 * nq) abort();   // l_m holds 1024 columns
    const long rows = 4L * EV_UNROLL * (nq <= 64 ? 64 / nq : 1);       // rows of one trip of a workgroup
    const dim3 grid((unsigned)std::min<long>(EV_MAX_WG, ((long)P.num_item + rows - 1) / rows));
    if (nq <= 64) hipLaunchKernelGGL(k_rank_item_envelope<1>, grid, dim3(256), 0, st, P, item_rows, item_bias, envelope);
    else if (nq <= 128) hipLaunchKernelGGL(k_rank_item_envelope<2>, grid, dim3(256), 0, st, P, item_rows, item_bias, envelope);
    else hipLaunchKernelGGL(k_rank_item_envelope<4>, grid, dim3(256), 0, st, P, item_rows, item_bias, envelope);
}

__global__ __launch_bounds__(64) void k_rank_topn_exact(const DevParams P, const RankTopnDev D) {
    __shared__ tn_key_t l_app[TN_SORT];   // the section's largest approximate keys, in rank order once merged
    __shared__ tn_key_t l_pin[TN_SORT];   // the pinned keys of the same candidates
    __shared__ float4 l_rows[64 * TX_LP];
    __shared__ float4 l_u[256];
    const int sec = blockIdx.x, lane = threadIdx.x, N = D.exact_n, M = D.top_n;
    const int k = P.k, nq = P.pitch >> 2;
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);

    // ---- the M largest approximate keys over the section's gy lists: k_rank_topn_merge's streaming with M for N
    const tn_key_t below = (1ull << lane) - 1ull;
    int cnt = 0;
    tn_key_t thr = 0ull;
    const bool bad = D.nan_cnt[sec] != 0;   // (c): the matrix sweep flagged a NaN
    if (!bad)
        for (int y = 0; y < D.gy; y++) {
            const int n = D.list_cnt[(size_t)sec * D.gy + y];
            const tn_key_t *list = D.list + ((size_t)sec * D.gy + y) * D.cap;
            for (int i0 = 0; i0 < n; i0 += 64) {
                if (cnt + 64 > TN_SORT) cnt = tn_sort_keep(l_app, cnt, M, lane, thr);
                const tn_key_t key = i0 + lane < n ? list[i0 + lane] : 0ull;
                const bool take = key > thr;
                const tn_key_t b = __ballot(take);
                if (take) l_app[cnt + __popcll(b & below)] = key;
                cnt += __popcll(b);
                tn_wave_sync();
            }
        }
    cnt = tn_sort_keep(l_app, cnt, M, lane, thr);

    // ---- u, once: into LDS for the chains; H_s and (a) for u in float64
    const float4 *urow = re_section_row(P, D.user_rows, D.sec_user, sec);
    double h = 0.0;
    unsigned uflags = 0u;
    for (int q = lane; q < nq; q += 64) {
        const float4 u = urow[q];
        l_u[q] = u;
        const float ue[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (4 * q + e < k) {
                const unsigned ab = __float_as_uint(ue[e]) & EV_ABS;
                uflags |= ev_flags(ab);
                h += (double)__uint_as_float(ab) * (double)__uint_as_float(D.envelope[4 * q + e]);
            }
    }
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off);
    const double H = (double)__uint_as_float(D.envelope[RANK_ENV_BIAS]) + h;
    const double delta = 4.0 * (double)(k + 2) * 0x1p-24 * H + (double)(k + 2) * 0x1p-124;
    // (a), (b), (c); a NaN or inf in H fails the comparison
    bool cert = !bad && D.envelope[RANK_ENV_FLAGS] == 0u && __ballot(uflags != 0u) == 0ull && H <= 0x1p126;
    tn_wave_sync();

    // ---- the pinned scores of the listed candidates, 64 at a time, K in chunks through LDS
    bool pnan = false;
    for (int r0 = 0; r0 < cnt; r0 += 64) {
        const int ci = r0 + lane;
        bool on;
        int id;
        const float s = tx_pinned_scores(P, ibase, ibias, l_u, l_rows, r0, cnt, lane, [&](int i) { return tn_key_id(l_app[i]); }, on, id);
        if (on) {
            pnan = pnan || s != s;
            l_pin[ci] = s == s ? tn_key(s, id) : 0ull;   // a NaN leaves the section to the pinned sweep, which flags it
        }
    }
    tn_wave_sync();
    tn_key_t pthr = 0ull;
    const int keep = tn_sort_keep(l_pin, cnt, N, lane, pthr);
    cert = cert && __ballot(pnan) == 0ull;
    // (d): fewer than M keys: every ranked candidate is listed; else the N-th pinned score must clear the last kept approximate score
    if (cert && cnt >= M) cert = (double)tn_key_score(l_pin[N - 1]) > (double)tn_key_score(l_app[M - 1]) + delta;
    for (int r = lane; r < N; r += 64) {
        const tn_key_t key = r < keep ? l_pin[r] : 0ull;
        D.item_out[(size_t)sec * N + r] = r < keep ? tn_key_id(key) : -1;
        D.score_out[(size_t)sec * N + r] = r < keep ? tn_key_score(key) : 0.0f;
    }
    if (lane == 0) {
        D.count_out[sec] = keep;
        D.certified[sec] = cert ? 1 : 0;
    }
}

void launch_rank_topn_exact(const DevParams &P, const RankTopnDev &D, hipStream_t st) {
    // M keys are kept and sorted in one wave's buffer, the N-th of them is read: another pair would read past it; l_u holds 256 float4s
    if (D.nsec <= 0 || D.exact_n < 1 || D.top_n <= D.exact_n || D.top_n > TN_SORT || (P.pitch >> 2) > 256 || !D.envelope || !D.certified) abort();
    hipLaunchKernelGGL(k_rank_topn_exact, dim3((unsigned)D.nsec), dim3(64), 0, st, P, D);
}

}  // namespace svdf

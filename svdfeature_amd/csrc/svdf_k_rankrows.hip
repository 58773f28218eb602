// svdf_k_rankrows.hip -- the effective user rows of the batch ranking calls on a user-group (SVD++) trainer.
//
// The ranker scores a user-group section with tmp_ufactor = tmp_ufeedback + W_user[u] * 1, where tmp_ufeedback = 0 + sum_j W_ufeedback[fid_j]
// * val_j in list order (apex_svd_base.h:719-735, 798-808): k_rank_feedback followed by k_rank_user (svdf_k_rank.hip), one section per
// launch.  k_rank_live_rows forms that row for every section of a piece in one launch, with those kernels' operations -- axpy4: unfused
// multiply, then add, per element a serial fp32 chain in list order -- and writes it to a workspace [nsec][pitch] that the sweeps of
// svdf_k_rankeval.hip / svdf_k_ranktopn.hip read in place of W_user rows.  One lane group (LPI lanes, one float4 each; a whole wave with
// 2 .. 4 float4 per lane for wide rows) owns a section, 64 / LPI sections share a wave.  A list's chain is serial by contract, so a list
// is never split over waves: a long list costs its length.  The row loads of a list do not depend on each other: RR_NB rows are requested
// together ahead of their adds.  Plain vector loads and stores; no LDS, no atomics.
#include "svdf_device.h"

namespace svdf {

constexpr int RR_NB = 8;   // feedback rows requested at a time (8 x 16 floats per lane for the widest rows: no scratch)

// A NaN VALUE is the one input on which the batch call leaves the ranker: the reference's scalar_map takes a NaN scalar for 1 (its
// |s - 1| > 1e-6 test is false, svdf_device.h: scalar_is_one), so the ranker would add the row unscaled and say nothing.  Here the NaN
// reaches every element of the section's row -- f + NaN -- and flags the section like any NaN score.
__device__ __forceinline__ void rr_poison(float4 &f, float nan) { f.x = f.x + nan; f.y = f.y + nan; f.z = f.z + nan; f.w = f.w + nan; }
template <int V> __device__ __forceinline__ void rr_poison(WideRow<V> &f, float nan) {
#pragma unroll
    for (int v = 0; v < V; v++) rr_poison(f.v[v], nan);
}

template <int LPI, typename R>
__global__ __launch_bounds__(256) void k_rank_live_rows(const DevParams P, const RankLiveRowsDev D) {
    using io = row_io<LPI, R>;
    constexpr int SPW = 64 / LPI;   // sections of a wave
    const int lane = threadIdx.x & 63, L = lane & (LPI - 1);
    const long sec = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SPW + lane / LPI;
    if (sec >= D.nsec) return;
    const int b = D.fb_p0[sec], e = D.fb_p0[sec + 1];
    const R urow = io::load(P.W, P.user_off + D.sec_user[sec], P.pitch, L, P.k);   // in flight under the whole list
    R f = row_traits<R>::zero();
    for (int t = b; t < e; t += RR_NB) {
        R r[RR_NB];
        float v[RR_NB];
#pragma unroll
        for (int q = 0; q < RR_NB; q++) {
            const bool in = t + q < e;
            r[q] = in ? io::load(P.W, P.fb_off + D.fb_index[t + q], P.pitch, L, P.k) : row_traits<R>::zero();
            v[q] = in ? D.fb_value[t + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < RR_NB; q++)
            if (t + q < e) {   // a row past the list is not added: x + 0 * 0 is not x for x = -0
                axpy4(f, r[q], v[q]);
                if (v[q] != v[q]) rr_poison(f, v[q]);
            }
    }
    axpy4(f, urow, 1.0f);   // proc_user on top of tmp_ufeedback: the USER line u:1
    io::store(D.rows, (size_t)sec, P.pitch, L, P.k, f);
}

void launch_rank_live_rows(const DevParams &P, const RankLiveRowsDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    SVDF_DISPATCH_ROW(P.k, {
        const long per_block = 4L * (64 / LPI);
        hipLaunchKernelGGL((k_rank_live_rows<LPI, R>), dim3((unsigned)((D.nsec + per_block - 1) / per_block)), dim3(256), 0, st, P, D);
    });
}

}  // namespace svdf

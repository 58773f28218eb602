// svdf_k_itemrows.hip -- the item side of svdf_item_topn: similar-item lists on the live model.
//
// The selecting sweeps of svdf_k_ranktopn.hip score a section with one row of a workspace against every row of an item matrix; an item
// call hands them item rows on BOTH sides.  Two small kernels prepare that:
//   k_item_unit_rows   the unit rows R of the cosine metric, once per call: for every item i, ss = <W_item[i], W_item[i]> in the pinned
//                      order (group_dot, identical on every lane of the group), n = sqrt(ss), R[i][j] = W_item[i][j] / n -- the correctly
//                      rounded square root and a correctly rounded DIVISION per element (the build's
//                      -fhip-fp32-correctly-rounded-divide-sqrt; denormals kept), never a reciprocal; ss == 0 gives R[i] = +0.
//   k_item_query_rows  row item[s] of the base matrix (W_item for dot, R for cosine) into row s of the [nsec][pitch] workspace the sweeps
//                      read as user_rows.
// Both have k_rank_live_items' shape: one lane group (LPI lanes, one float4 each; a whole wave with 2 .. 4 float4 per lane for wide rows)
// per row, row_io loads and stores.  Plain vector loads and stores; no LDS, no atomics.
#include <algorithm>

#include "svdf_device.h"

namespace svdf {

// chunk c (elements 4 c .. 4 c + 3) of a row divided by n element by element; all of it +0 where `zero` is set; elements at or past k
// (the pad of the last chunk) stay +0 whatever n is
__device__ __forceinline__ float4 ir_unit_chunk(const float4 f, float n, bool zero, int c, int k) {
    float4 r;
    r.x = (zero || 4 * c >= k) ? 0.0f : f.x / n;
    r.y = (zero || 4 * c + 1 >= k) ? 0.0f : f.y / n;
    r.z = (zero || 4 * c + 2 >= k) ? 0.0f : f.z / n;
    r.w = (zero || 4 * c + 3 >= k) ? 0.0f : f.w / n;
    return r;
}
__device__ __forceinline__ float4 ir_unit(const float4 &f, float n, bool zero, int L, int k) { return ir_unit_chunk(f, n, zero, L, k); }
template <int V> __device__ __forceinline__ WideRow<V> ir_unit(const WideRow<V> &f, float n, bool zero, int L, int k) {
    WideRow<V> r;
#pragma unroll
    for (int v = 0; v < V; v++) r.v[v] = ir_unit_chunk(f.v[v], n, zero, L + 64 * v, k);
    return r;
}

// One lane group per item, grid-stride; `unit` has W_item's layout ([num_item][pitch], pads 0).  The trip count is uniform over a wave
// (the wave's groups step together and a group past the last item keeps walking with its lanes' work masked): group_dot crosses lanes.
template <int LPI, typename R>
__global__ __launch_bounds__(256) void k_item_unit_rows(const DevParams P, float *unit) {
    using io = row_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63, L = lane & (LPI - 1);
    const long wave_first = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW;
    const long stride = (long)gridDim.x * (blockDim.x >> 6) * IPW;
    for (long i0 = wave_first; i0 < (long)P.num_item; i0 += stride) {
        const long i = i0 + lane / LPI;
        const bool in = i < (long)P.num_item;
        const R f = in ? io::load(P.W, P.item_off + (size_t)i, P.pitch, L, P.k) : row_traits<R>::zero();
        const float ss = group_dot<LPI>(f, f, L, P.k);
        const float n = sqrtf(ss);
        const R r = ir_unit(f, n, ss == 0.0f, L, P.k);   // a select, not a branch around the store
        if (in) io::store(unit, (size_t)i, P.pitch, L, P.k, r);
    }
}

void launch_item_unit_rows(const DevParams &P, float *unit, hipStream_t st) {
    if (P.num_item <= 0) return;
    SVDF_DISPATCH_ROW(P.k, {
        const long per_block = 4L * (64 / LPI);
        const long blocks = std::min<long>(((long)P.num_item + per_block - 1) / per_block, 8192);
        hipLaunchKernelGGL((k_item_unit_rows<LPI, R>), dim3((unsigned)blocks), dim3(256), 0, st, P, unit);
    });
}

// One lane group per section: rows[s] = base[item[s]], `base` a [num_item][pitch] matrix.  No lane talks to another.
template <int LPI, typename R>
__global__ __launch_bounds__(256) void k_item_query_rows(const DevParams P, const float *__restrict__ base, const unsigned *__restrict__ item, int nsec,
                                                         float *__restrict__ rows) {
    using io = row_io<LPI, R>;
    constexpr int SPW = 64 / LPI;
    const int lane = threadIdx.x & 63, L = lane & (LPI - 1);
    const long sec = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SPW + lane / LPI;
    if (sec >= nsec) return;
    io::store(rows, (size_t)sec, P.pitch, L, P.k, io::load(base, (size_t)item[sec], P.pitch, L, P.k));
}

void launch_item_query_rows(const DevParams &P, const float *base, const unsigned *item, int nsec, float *rows, hipStream_t st) {
    if (nsec <= 0) return;
    SVDF_DISPATCH_ROW(P.k, {
        const long per_block = 4L * (64 / LPI);
        const dim3 grid((unsigned)((nsec + per_block - 1) / per_block));
        hipLaunchKernelGGL((k_item_query_rows<LPI, R>), grid, dim3(256), 0, st, P, base, item, nsec, rows);
    });
}

}  // namespace svdf

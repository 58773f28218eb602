// svdf_k_pairorder.hip -- the rows of a SHUFFLED pass of rank pairs from a pair source: one lane per position p
// computes sigma(p) (svdf_pairorder_lists.h; the rule is stated in include/svdfeature_amd.h) and gathers (user[sigma(p)], pos[sigma(p)]) into
// two scratch columns of n words, which k_pair_draw / k_pair_hard then read as the source's rows -- those kernels are unchanged, so a shuffled
// pass is the plain pass on the permuted rows by construction.  A position depends on nothing but (order_seed, n, p): no table, no sort.
// The walk's bound is the compile-time constant PAIR_ORDER_WALKS, so no input makes the kernel run long; a position that exhausts it is
// reported through a one-word flag (plain store, any writer may win) and gathers row 0, which is in bounds.
// The kernel also counts the positions whose user is the user of the position before -- the one fact about the permuted order that the route
// decision of a pass needs (PairSource::same for the caller's order).  The neighbour's user comes from the adjacent lane; the first lane of
// a wave recomputes sigma(p - 1).  The count is an integer sum: a popcount per wave, the four of a block added in LDS, one atomic add per
// block -- the same total in whatever order the blocks arrive.
#include "svdf_kernels.h"

namespace svdf {

__global__ __launch_bounds__(256) void k_pair_order(const PairOrderDev D) {
    __shared__ unsigned part[4];
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = p < D.n;
    unsigned u = 0u;
    if (live) {
        unsigned row;
        if (!pair_order_sigma(D.K, D.n, p, PAIR_ORDER_WALKS, &row)) *D.flag = (unsigned)(p + 1);   // (row = 0)
        u = D.user[row];
        D.out_user[p] = u;
        D.out_pos[p] = D.pos[row];
    }
    unsigned before = __shfl_up(u, 1);   // (a live lane's predecessor in the wave is live)
    if (lane == 0 && live && p > 0) {
        unsigned row;
        pair_order_sigma(D.K, D.n, p - 1, PAIR_ORDER_WALKS, &row);   // (position p - 1 reports its own exhaustion)
        before = D.user[row];
    }
    const unsigned long long m = __ballot(live && p > 0 && u == before);
    if (lane == 0) part[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = (part[0] + part[1]) + (part[2] + part[3]);
        if (s) atomicAdd(D.same, s);
    }
}

void launch_pair_order(const PairOrderDev &D, hipStream_t st) {
    if (D.n <= 0) return;
    hipLaunchKernelGGL(k_pair_order, dim3((unsigned)((D.n + 255) / 256)), dim3(256), 0, st, D);
}

}  // namespace svdf

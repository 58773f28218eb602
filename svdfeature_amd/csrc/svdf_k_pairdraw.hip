// svdf_k_pairdraw.hip -- the negatives of a pass of rank pairs, drawn on the device from a pair source: one lane per
// pair q = r * num_neg + j writes (user_r, pos_r, neg_q) into the pass's three columns, neg_q the first id of the pair's draw sequence
// (svdf_pairsource_lists.h; the rule is stated in include/svdfeature_amd.h) that is not among the distinct items of user_r -- a binary search
// in the user's ascending list.  A pair depends on nothing but (seed, q, its user's list): no atomics, nothing depends on timing.  The loop
// bound is the compile-time constant PAIR_SRC_DRAWS, so no input makes the kernel run long; the density rule the host applied when the
// source was created makes exhausting it a < 1e-28 event, reported through a one-word flag (plain store, any writer may win).
// Adjacent lanes belong to one row or to neighbouring rows: in a user-grouped source they search the same list, and the first probes of every
// search (the middle of the list, its quarters) are the same cache lines for the whole wave.
#include "svdf_kernels.h"
#include "svdf_pairsource_lists.h"

namespace svdf {

__global__ __launch_bounds__(256) void k_pair_draw(const PairDrawDev D) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= D.npair) return;
    const unsigned r = (unsigned)q / (unsigned)D.num_neg;   // (npair < 2^31)
    const unsigned u = D.user[r];
    const int p0 = D.uptr[u], p1 = D.uptr[u + 1];
    unsigned neg;
    if (!pair_src_pick(D.seed, (uint64_t)q, D.num_item, D.uitems, p0, p1, PAIR_SRC_DRAWS, &neg)) *D.flag = (unsigned)(q + 1);
    if (D.out_user) {
        D.out_user[q] = u;
        D.out_pos[q] = D.pos[r];
    }
    D.out_neg[q] = neg;
}

void launch_pair_draw(const PairDrawDev &D, hipStream_t st) {
    if (D.npair <= 0) return;
    hipLaunchKernelGGL(k_pair_draw, dim3((unsigned)((D.npair + 255) / 256)), dim3(256), 0, st, D);
}

}  // namespace svdf

// svdf_k_pairdraw.hip -- the negatives of a pass of rank pairs, drawn on the device from a pair source: one lane per
// pair q = r * num_neg + j writes (user_r, pos_r, neg_q) into the pass's three columns, neg_q the first id of the pair's draw sequence
// (svdf_pairsource_lists.h; the rule is stated in include/svdfeature_amd.h) that is not among the distinct items of user_r -- a binary search
// in the user's ascending list.  A pair depends on nothing but (seed, q, its user's list): no atomics, nothing depends on timing.  The loop
// bound is the compile-time constant PAIR_SRC_DRAWS, so no input makes the kernel run long; the density rule the host applied when the
// source was created makes exhausting it a < 1e-28 event, reported through a one-word flag (plain store, any writer may win).
// Adjacent lanes belong to one row or to neighbouring rows: in a user-grouped source they search the same list, and the first probes of every
// search (the middle of the list, its quarters) are the same cache lines for the whole wave.
// A source with ITEM WEIGHTS (section 6ae) draws through its weight table instead of the multiply: WF = 1 searches the whole cdf per draw,
// WF = 2 between the two guide entries of the word's bucket (svdf_pairweight_lists.h; equal ids).  WF is a template argument, so the
// unweighted kernel (WF = 0) holds no trace of the table.  The same file holds the one-launch probe of the map, k_pair_weight_lookup.
#include "svdf_kernels.h"
#include "svdf_pairweight_lists.h"

namespace svdf {

template <int WF>
__global__ __launch_bounds__(256) void k_pair_draw(const PairDrawDev D, const PairWeightDev T) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= D.npair) return;
    const unsigned r = (unsigned)q / (unsigned)D.num_neg;   // (npair < 2^31)
    const unsigned u = D.user[r];
    const int p0 = D.uptr[u], p1 = D.uptr[u + 1];
    unsigned neg;
    int took;
    if constexpr (WF == 0) took = pair_src_pick(D.seed, (uint64_t)q, D.num_item, D.uitems, p0, p1, PAIR_SRC_DRAWS, &neg);
    else took = pair_weight_pick<WF>(D.seed, (uint64_t)q, T, D.uitems, p0, p1, PAIR_SRC_DRAWS, &neg);
    if (!took) *D.flag = (unsigned)(q + 1);
    if (D.out_user) {
        D.out_user[q] = u;
        D.out_pos[q] = D.pos[r];
    }
    D.out_neg[q] = neg;
}

// the probe svdf_pair_weight_lookup: lane j maps the word x[j]
template <int WF>
__global__ __launch_bounds__(256) void k_pair_weight_lookup(const PairWeightDev T, const long nx, const uint64_t *x, unsigned *id_out) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j < nx) id_out[j] = pair_weight_lookup<WF>(T, x[j]);
}

// The measured choice of the weighted form (profiles/r36_pair_weight.md: 20 M pairs, 10 K and 100 K items, Zipf and equal weights, k_pair_draw
// and k_pair_hard at num_cand 8): the guided search won by more than both spreads in every cell at 10 K items, the search of the whole cdf in
// three of the four cells at 100 K items (the fourth inside the spreads).  A catalogue takes the column of the next measured size above it.
constexpr long PAIR_WEIGHT_GUIDED_ITEMS = 10000;
int pair_weight_form(long num_item, int form) {
    if (form == 1 || form == 2) return form;
    return num_item <= PAIR_WEIGHT_GUIDED_ITEMS ? 2 : 1;
}

void launch_pair_draw(const PairDrawDev &D, const PairWeightDev &T, int wform, hipStream_t st) {
    if (D.npair <= 0) return;
    const dim3 grid((unsigned)((D.npair + 255) / 256));
    if (!T.cdf) hipLaunchKernelGGL(k_pair_draw<0>, grid, dim3(256), 0, st, D, T);
    else if (pair_weight_form((long)T.num_item, wform) == 2) hipLaunchKernelGGL(k_pair_draw<2>, grid, dim3(256), 0, st, D, T);
    else hipLaunchKernelGGL(k_pair_draw<1>, grid, dim3(256), 0, st, D, T);
}

void launch_pair_weight_lookup(const PairWeightDev &T, int wform, long nx, const uint64_t *x, unsigned *id_out, hipStream_t st) {
    if (nx <= 0) return;
    const dim3 grid((unsigned)((nx + 255) / 256));
    if (pair_weight_form((long)T.num_item, wform) == 2) hipLaunchKernelGGL(k_pair_weight_lookup<2>, grid, dim3(256), 0, st, T, nx, x, id_out);
    else hipLaunchKernelGGL(k_pair_weight_lookup<1>, grid, dim3(256), 0, st, T, nx, x, id_out);
}

}  // namespace svdf

// svdf_k_rankwin.hip -- the window rule of a window sequence (DESIGN.md sections 6a, 6r) evaluated ON THE DEVICE, for a pass of rank pairs the
// device sampler left in HBM (svdf_k_sample.hip; Engine::wseq_from_device_pairs).
//
// The host builder (wseq_from_pairs) reads the pass's columns three times: the per-item counts, the per-pass window count, and the raise of that
// count on the windows as they are cut.  Here the columns never leave HBM:
//   * k_rw_columns turns the sampler's merged, index-sorted item entries (i0, v0, i1: the negative's value sign-flipped) back into the positive and
//     the negative item of every pair -- what window_build_resident takes --, checks the ids like k_wb_item_keys does, and counts every item's
//     entries with integer atomics (order-independent);
//   * one stable radix sort (rocPRIM) orders the 2 n entries by item, positions ascending inside an item, ONCE per pass;
//   * k_rw_window_sums then gives, for a candidate window count W, the two integers the rule is made of: the sum over (item, window) of c^2 -- c
//     the item's entries in the window [n w / W, n (w + 1) / W); the sum over entries of their running count's 2 v - 1 that WseqCounter adds up --
//     and the largest c.  Inside an item the positions ascend, so (item, window) is non-decreasing along the sorted entries: a run's first entry
//     finds its end by bisection.  Integer sums: the same excess(), the same W as the host search, whatever the order of the atomics.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "svdf_kernels.h"

namespace svdf {

namespace {

inline unsigned rw_grid(long n) {
    long g = (n + 255) / 256;
    return (unsigned)std::max<long>(1, std::min<long>(g, 1L << 16));
}
inline int rw_bits(unsigned long long v) {
    int b = 1;
    while (b < 64 && (v >> b) != 0ull) b++;
    return b;
}

// MERGED = false: the columns ARE the positive and the negative item of every pair (a pair source's draw, svdf_pairsource.cpp): i0 = pos, i1 = neg,
// v0 / pos / neg unused -- the same checks, counts and keys.
template <bool MERGED>
__global__ __launch_bounds__(256) void k_rw_columns(long n, const unsigned *user, const unsigned *i0, const float *v0, const unsigned *i1, unsigned NU, unsigned NI,
                                                    unsigned *pos, unsigned *neg, unsigned *keys, unsigned *vals, unsigned *count, unsigned *state) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const unsigned a = i0[r], b = i1[r];
        unsigned err = 0u;
        if (user[r] >= NU) err |= (unsigned)RW_ERR_USER;
        if (MERGED ? b == SLOT_ABSENT : a == b) err |= (unsigned)RW_ERR_SAME;   // positive and negative row name one item: the merged row has ONE entry (apex_svd_data.cpp:828-860)
        else if (b >= NI) err |= (unsigned)RW_ERR_ITEM;
        if (a >= NI) err |= (unsigned)RW_ERR_ITEM;
        const bool first_pos = !MERGED || v0[r] > 0.0f;   // unit values: entry 0 is +1 (the positive's) or -1 (the negative's, sign flipped)
        unsigned p = first_pos ? a : b, q = first_pos ? b : a;
        if (err) { atomicOr(&state[0], err); p = 0u; q = 0u; }
        else { atomicAdd(&count[p], 1u); atomicAdd(&count[q], 1u); }
        if (MERGED) { pos[r] = p; neg[r] = q; }
        if (keys) { keys[2 * r] = p; keys[2 * r + 1] = q; vals[2 * r] = (unsigned)(2 * r); vals[2 * r + 1] = (unsigned)(2 * r + 1); }
    }
}

// the window of file position r when n positions are cut into W windows [n w / W, n (w + 1) / W): the largest w with n w / W <= r
__device__ __forceinline__ long rw_window(long r, long n, long W) { return ((r + 1) * W - 1) / n; }

__global__ __launch_bounds__(256) void k_rw_window_sums(const unsigned *item, const unsigned *entry, long E, long n, long W, unsigned long long *out) {
    __shared__ unsigned long long s_sum[256], s_max[256];
    const long stride = (long)gridDim.x * blockDim.x;
    unsigned long long sum = 0ull, worst = 0ull;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < E; p += stride) {
        const unsigned it = item[p];
        const long w = rw_window((long)(entry[p] >> 1), n, W);
        if (p > 0 && item[p - 1] == it && rw_window((long)(entry[p - 1] >> 1), n, W) == w) continue;   // not the first entry of its (item, window) run
        long lo = p + 1, hi = E;   // first entry past the run
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            if (item[mid] == it && rw_window((long)(entry[mid] >> 1), n, W) == w) lo = mid + 1; else hi = mid;
        }
        const unsigned long long c = (unsigned long long)(lo - p);
        sum += c * c;
        worst = c > worst ? c : worst;
    }
    s_sum[threadIdx.x] = sum; s_max[threadIdx.x] = worst;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
            if (s_max[threadIdx.x + h] > s_max[threadIdx.x]) s_max[threadIdx.x] = s_max[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(&out[0], s_sum[0]);
        if (s_max[0]) atomicMax(&out[1], s_max[0]);
    }
}

#define RWCHK(call)                                                                                                   \
    do {                                                                                                              \
        hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess) throw std::runtime_error(std::string("device window rule: ") + hipGetErrorString(e_) + " at " #call); \
    } while (0)

}  // namespace

void launch_rank_window_columns(long n, const unsigned *user, const unsigned *i0, const float *v0, const unsigned *i1, long num_user, long num_item,
                                unsigned *pos, unsigned *neg, unsigned *keys, unsigned *vals, unsigned *count, unsigned *state, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rw_columns<true>, dim3(rw_grid(n)), dim3(256), 0, st, n, user, i0, v0, i1, (unsigned)num_user, (unsigned)num_item, pos, neg, keys, vals, count, state);
}
void launch_rank_window_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg, long num_user, long num_item, unsigned *keys, unsigned *vals,
                              unsigned *count, unsigned *state, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rw_columns<false>, dim3(rw_grid(n)), dim3(256), 0, st, n, user, pos, (const float *)nullptr, neg, (unsigned)num_user, (unsigned)num_item,
                       (unsigned *)nullptr, (unsigned *)nullptr, keys, vals, count, state);
}

size_t rank_window_sort_bytes(long E) {
    size_t a = 0;
    RWCHK(rocprim::radix_sort_pairs(nullptr, a, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr, (unsigned *)nullptr, (size_t)E, 0u, 32u, hipStream_t(0)));
    return a;
}
void rank_window_sort(void *tmp, size_t tmp_bytes, const unsigned *keys, unsigned *keys_sorted, const unsigned *vals, unsigned *vals_sorted, long E, long num_item,
                      hipStream_t st) {
    if (E <= 0) return;
    size_t tb = tmp_bytes;
    RWCHK(rocprim::radix_sort_pairs(tmp, tb, keys, keys_sorted, vals, vals_sorted, (size_t)E, 0u, (unsigned)rw_bits((unsigned long long)std::max<long>(num_item, 1)), st));
}
// out[0] = sum of c^2, out[1] = max c over the (item, window) runs of the sorted entries; one 16-byte read-back
void rank_window_sums(const unsigned *keys_sorted, const unsigned *vals_sorted, long E, long n, long W, unsigned long long *d_out, unsigned long long *sum,
                      unsigned long long *worst, hipStream_t st) {
    unsigned long long h[2] = {0ull, 0ull};
    RWCHK(hipMemsetAsync(d_out, 0, sizeof(h), st));
    hipLaunchKernelGGL(k_rw_window_sums, dim3(rw_grid(E)), dim3(256), 0, st, keys_sorted, vals_sorted, E, n, W, d_out);
    RWCHK(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, st));
    RWCHK(hipStreamSynchronize(st));
    RWCHK(hipGetLastError());
    *sum = h[0]; *worst = h[1];
}

}  // namespace svdf

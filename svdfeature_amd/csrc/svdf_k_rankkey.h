// svdf_k_rankkey.h -- the 64-bit rank key of a (score, item id) pair and the wave's LDS sort over such keys, shared by the top-N kernels
// (svdf_k_ranktopn.hip; svdf_k_rankcand.hip, section 6aa): (order-preserving word of the score) << 32 | ~id, so that a
// larger key is a better rank (higher score first, equal scores by ascending id, -0 folded onto +0) and the keys of a section are distinct.
#ifndef SVDF_K_RANKKEY_H_
#define SVDF_K_RANKKEY_H_

#include "svdf_kernels.h"

namespace svdf {

constexpr int TN_SORT = RANK_TOPN_MAX_CAP;   // keys of a wave's sort buffer
typedef unsigned long long tn_key_t;         // 0: no key (smaller than every key: -inf maps to word 0x007fffff, NaNs are never keyed)

__device__ __forceinline__ tn_key_t tn_key(float s, int id) {
    unsigned b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;   // -0 == +0
    const unsigned w = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((tn_key_t)w << 32) | (tn_key_t)(~(unsigned)id);
}
__device__ __forceinline__ float tn_key_score(tn_key_t key) {
    const unsigned w = (unsigned)(key >> 32);
    return __uint_as_float((w & 0x80000000u) ? (w & 0x7fffffffu) : ~w);
}
__device__ __forceinline__ int tn_key_id(tn_key_t key) { return (int)(~(unsigned)key); }

// the lanes of ONE wave hand LDS values to each other: LDS operations of a wave complete in order; this keeps the compiler from moving them
__device__ __forceinline__ void tn_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// buf[0 .. cnt) (cnt <= TN_SORT, one wave's LDS) sorted descending by a bitonic network over the next power of two (zeros fill the rest);
// returns how many keys stay, min(cnt, top_n), and raises thr to the smallest of them once there are top_n
__device__ __forceinline__ int tn_sort_keep(tn_key_t *buf, int cnt, int top_n, int lane, tn_key_t &thr) {
    int n2 = 64;
    while (n2 < cnt) n2 <<= 1;
    for (int i = cnt + lane; i < n2; i += 64) buf[i] = 0ull;
    tn_wave_sync();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (n2 >> 1); t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const tn_key_t x = buf[lo], y = buf[hi];
                if ((x < y) == desc) { buf[lo] = y; buf[hi] = x; }
            }
            tn_wave_sync();
        }
    const int keep = cnt < top_n ? cnt : top_n;
    if (cnt >= top_n) thr = buf[top_n - 1];
    return keep;
}

}  // namespace svdf
#endif

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

// ---- deep lists (top_n 257 .. 4096, knob rank_topn_deep): a list of up to RANK_TOPN_DEEP_MAX_CAP keys does not fit a
// wave's sort buffer, so it is cut where it lies, in the HBM workspace (L2-resident), by a radix SELECT: the keys are distinct, so the
// top_n-th largest is an exact threshold and exactly top_n keys are at or above it.
constexpr int TN_HIST = 256;   // bins of one pass: one byte of the key; a wave's histogram in LDS
constexpr int tn_scratch_keys(bool deep) { return deep ? TN_HIST / 2 : TN_SORT; }   // the wave's LDS scratch, in keys: a histogram or a sort buffer

// the bin that holds the want-th largest key (1 <= want <= the bins' sum) counted from bin 255 down, by a wave scan: lane l owns the bins
// 255 - 4 l .. 252 - 4 l.  want becomes the rank inside that bin.
__device__ __forceinline__ int tn_hist_pick(const int *hist, int lane, int &want) {
    int c[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) { c[q] = hist[255 - 4 * lane - q]; sum += c[q]; }
    int upto = sum;   // inclusive prefix over the lanes
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(upto, d);
        upto += lane >= d ? y : 0;
    }
    int above = upto - sum, bin = 0, rest = 0;
    const bool here = above < want && want <= upto;   // one lane
#pragma unroll
    for (int q = 0; q < 4; q++) {   // (no indexed register array: the first bin that reaches want)
        if (rest == 0 && want <= above + c[q]) { bin = 255 - 4 * lane - q; rest = want - above; }
        above += c[q];
    }
    const int src = __ffsll((unsigned long long)__ballot(here)) - 1;
    want = __shfl(rest, src);
    return __shfl(bin, src);
}

// list[0 .. cnt) (one wave's list in global memory) cut IN PLACE to its top_n largest keys, unordered: eight passes, most significant byte
// first, each a histogram of that byte over the keys that match the bytes found so far; then the keys at or above the threshold are moved
// to the front, 64 at a time -- a chunk is in registers before any lane writes, and the write cursor never passes the read cursor.  Returns
// how many keys stay, min(cnt, top_n), and raises thr to the smallest of them once there are top_n (tn_sort_keep's contract).
__device__ __forceinline__ int tn_select_keep(tn_key_t *list, int cnt, int top_n, int lane, int *hist, tn_key_t &thr) {
    if (cnt < top_n) return cnt;
    tn_key_t prefix = 0ull, mask = 0ull;
    int want = top_n;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int q = lane; q < TN_HIST; q += 64) hist[q] = 0;
        tn_wave_sync();
        for (int i = lane; i < cnt; i += 64) {
            const tn_key_t key = list[i];
            if ((key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
        }
        tn_wave_sync();
        const int bin = tn_hist_pick(hist, lane, want);
        prefix |= (tn_key_t)bin << shift;
        mask |= 0xffull << shift;
        tn_wave_sync();   // the bins have been read
    }
    thr = prefix;
    const tn_key_t below = (1ull << lane) - 1ull;
    int w = 0;
    for (int base = 0; base < cnt; base += 64) {
        const tn_key_t key = base + lane < cnt ? list[base + lane] : 0ull;
        const bool keep = key >= prefix;
        const tn_key_t b = __ballot(keep);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the chunk has been read by every lane
        if (keep) list[w + __popcll(b & below)] = key;          // w + popc(b) <= base + 64
        w += __popcll(b);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    return w;   // top_n
}

}  // namespace svdf
#endif

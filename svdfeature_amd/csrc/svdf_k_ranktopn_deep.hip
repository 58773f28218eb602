// svdf_k_ranktopn_deep.hip -- the merge of a deep top-N call (top_n 257 .. 4096, knob rank_topn_deep = 1).  The sweeps
// of such a call are the deep forms of k_rank_topn_sweep, k_rank_topn_sweep_wide (svdf_k_ranktopn.hip) and k_rank_topn_sweep_mfma
// (svdf_k_ranktopn_mfma.hip): the same scoring, lists of up to 8192 keys that the owning wave cuts where they lie (tn_select_keep,
// svdf_k_rankkey.h), kept in no order.  What a section's gy lists hold is a superset of its top_n largest keys.
//
// k_rank_topn_merge_deep: a workgroup of 256 threads owns a section.
//   select  the same radix select as the cut, over all the section's lists where they lie: eight passes, most significant byte first, one
//           histogram of 256 bins per workgroup in LDS (LDS atomics), thread t owning bin 255 - t in the scan from the top bin down; the
//           bytes found so far stay in registers.  The keys of a section are distinct, so exactly top_n of them are at or above the
//           threshold.  A section with no more than top_n keys keeps them all and skips the passes.
//   gather  the survivors go to LDS (at most 4096 keys, 32 KiB) through one LDS cursor, in no order;
//   sort    descending by a bitonic network over the next power of two (zeros fill the rest): compare distances below 64 by __shfl_xor on
//           a register (element e lives in lane e & 63 of the wave that owns its 64), larger ones as compare-exchanges in LDS, one barrier
//           per stage -- k_rank_cand_sets' network on 64-bit keys;
//   write   item_out / score_out / count_out and the padding, as k_rank_topn_merge writes them.
// No global atomics, no scratch.
#include <cstdlib>

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"

namespace svdf {

constexpr int TD_THREADS = 256;

// one compare-exchange of the descending network inside a wave: element e against element e ^ j, j < 64, in the merge of runs of length k
__device__ __forceinline__ tn_key_t td_step(tn_key_t v, int e, int k, int j) {
    const tn_key_t o = __shfl_xor(v, j);
    return ((e & j) == 0) == ((e & k) == 0) ? (v > o ? v : o) : (v < o ? v : o);
}

// key[0 .. P) in LDS, P a power of two >= 64, sorted descending by the whole workgroup; ends behind a barrier
__device__ __forceinline__ void td_sort(tn_key_t *key, int P, int tid) {
    for (int e = tid; e < P; e += TD_THREADS) {   // runs of up to 64 in registers (P is a multiple of 64: a wave is in or out as one)
        tn_key_t v = key[e];
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) v = td_step(v, e, k, j);
        key[e] = v;
    }
    for (int k = 128; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            __syncthreads();
            for (int p = tid; p < (P >> 1); p += TD_THREADS) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));   // pair p: elements i and i + j
                const tn_key_t a = key[i], b = key[i + j];
                if ((a < b) == ((i & k) == 0)) { key[i] = b; key[i + j] = a; }
            }
        }
        __syncthreads();
        for (int e = tid; e < P; e += TD_THREADS) {
            tn_key_t v = key[e];
            for (int j = 32; j > 0; j >>= 1) v = td_step(v, e, k, j);
            key[e] = v;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(TD_THREADS) void k_rank_topn_merge_deep(const RankTopnDev D) {
    __shared__ tn_key_t buf[RANK_TOPN_DEEP_MAX];
    __shared__ int hist[TN_HIST];
    __shared__ int wsum[TD_THREADS / 64];
    __shared__ int pick[2];   // the bin of a pass and the rank wanted inside it
    __shared__ int cursor;
    const int sec = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = D.top_n;
    const int *lcnt = D.list_cnt + (size_t)sec * D.gy;
    const tn_key_t *lists = D.list + (size_t)sec * D.gy * D.cap;
    const bool bad = D.nan_cnt[sec] != 0;   // a ranked candidate scored NaN: the section lists nothing
    long total = 0;
    if (!bad)
        for (int y = 0; y < D.gy; y++) total += lcnt[y];
    if (tid == 0) cursor = 0;

    // ---- the threshold: the N-th largest key where there are more than N; else every key (a key is never 0)
    tn_key_t prefix = 0ull, mask = 0ull;
    if (total > N) {   // workgroup-uniform
        int want = N;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int y = 0; y < D.gy; y++) {
                const int n = lcnt[y];
                const tn_key_t *list = lists + (size_t)y * D.cap;
                for (int i = tid; i < n; i += TD_THREADS) {
                    const tn_key_t key = list[i];
                    if ((key & mask) == prefix) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
                }
            }
            __syncthreads();
            const int c = hist[TN_HIST - 1 - tid];
            int upto = c;   // inclusive prefix from the top bin down: over the wave, then over the waves ahead
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(upto, d);
                upto += lane >= d ? y : 0;
            }
            if (lane == 63) wsum[wave] = upto;
            __syncthreads();
            for (int w = 0; w < wave; w++) upto += wsum[w];
            if (upto - c < want && want <= upto) { pick[0] = TN_HIST - 1 - tid; pick[1] = want - (upto - c); }   // one thread
            __syncthreads();
            prefix |= (tn_key_t)pick[0] << shift;
            mask |= 0xffull << shift;
            want = pick[1];
        }
    }
    __syncthreads();   // the cursor is zero, the last pick has been read

    // ---- the survivors, in no order: total <= N of them when nothing was selected, exactly N otherwise
    const int K = total < (long)N ? (int)total : N;
    for (int y = 0; y < D.gy && !bad; y++) {
        const int n = lcnt[y];
        const tn_key_t *list = lists + (size_t)y * D.cap;
        for (int i = tid; i < n; i += TD_THREADS) {
            const tn_key_t key = list[i];
            if (key >= prefix) {
                const int at = atomicAdd(&cursor, 1);
                if (at < RANK_TOPN_DEEP_MAX) buf[at] = key;   // (at < K: the keys of a section are distinct)
            }
        }
    }
    int P = 64;
    while (P < K) P <<= 1;
    __syncthreads();
    for (int e = K + tid; e < P; e += TD_THREADS) buf[e] = 0ull;
    __syncthreads();
    td_sort(buf, P, tid);

    for (int r = tid; r < N; r += TD_THREADS) {
        const tn_key_t key = r < K ? buf[r] : 0ull;
        D.item_out[(size_t)sec * N + r] = r < K ? tn_key_id(key) : -1;
        D.score_out[(size_t)sec * N + r] = r < K ? tn_key_score(key) : 0.0f;
    }
    if (tid == 0) D.count_out[sec] = K;
}

void launch_rank_topn_merge_deep(const RankTopnDev &D, hipStream_t st) {
    // buf holds top_n keys: a launch with a longer list would need more LDS than the kernel has
    if (D.nsec <= 0 || D.top_n < 1 || D.top_n > RANK_TOPN_DEEP_MAX) abort();
    hipLaunchKernelGGL(k_rank_topn_merge_deep, dim3((unsigned)D.nsec), dim3(TD_THREADS), 0, st, D);
}

}  // namespace svdf

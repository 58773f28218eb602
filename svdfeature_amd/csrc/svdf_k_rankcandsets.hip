// svdf_k_rankcandsets.hip -- the sections' ranked sets of the _cand calls, built on the device (knob rank_cand_build
// = 1): from a section's raw ids -- its candidates, then its positives, repeats and all -- to its distinct ids in ascending order, which is
// what the host's rank_cand_build (svdf_rankcand_lists.h) makes by sort + unique or by marking a bitmap.  Integers only: both forms below
// give the one set there is, so every result of the calls stays what the host build gives.
//
// k_rank_cand_sets: a workgroup of 256 threads owns a section; the section's form word (rank_cand_set_form, evaluated on the host) picks
//   the sort form   the ids go to LDS once, padded with 0xFFFFFFFF to a power of two >= 64, and a bitonic network sorts them: compare
//                   distances below 64 by __shfl_xor on a register (element e lives in lane e & 63 of the wave that owns its 64), larger
//                   ones as compare-exchanges in LDS, one barrier per stage;
//   the bitmap form one bit per item of the catalogue in LDS (up to 64 KiB), set by LDS atomics.
// Either way each wave then owns a contiguous quarter of the LDS image and walks it twice, 64 entries a round: once to count what it will
// write (heads of runs of equal keys / set bits), and, behind the exchange of the four wave totals, once to write it at its offset.  The set
// replaces the raw ids in place: every raw id has been read into LDS before the first is overwritten.
// k_rank_cand_pack: a wave per section copies the kept sets to their dense places and finds the positives' pairs by binary search.
#include <algorithm>

#include "svdf_kernels.h"

namespace svdf {

constexpr unsigned RCS_PAD = 0xFFFFFFFFu;   // no id: ids are below num_item <= 2^31
constexpr int RCS_THREADS = 256;

// The four waves' totals, through LDS without a word of LDS of its own (the bitmap may fill all 64 KiB): the words 0 .. 3 are saved in
// registers, lent to the totals and restored.  before: the totals of the waves ahead of this one; all: the four together.
__device__ inline void rcs_exchange(unsigned *lds, int total, int tid, int &before, int &all) {
    const int wave = tid >> 6;
    unsigned save = 0u;
    if (tid < 4) save = lds[tid];
    __syncthreads();
    if ((tid & 63) == 0) lds[wave] = (unsigned)total;
    __syncthreads();
    before = 0;
    all = 0;
    for (int w = 0; w < 4; w++) {
        const int t = (int)lds[w];
        all += t;
        before += w < wave ? t : 0;
    }
    __syncthreads();
    if (tid < 4) lds[tid] = save;
    __syncthreads();
}

// the chunks of 64 entries, of `chunks` in all, that wave `wave` owns: [c0, c1), a contiguous quarter
__device__ inline void rcs_quarter(int chunks, int wave, int &c0, int &c1) {
    const int per = (chunks + 3) >> 2;
    c0 = min(chunks, wave * per);
    c1 = min(chunks, (wave + 1) * per);
}

// one compare-exchange of the network inside a wave: element e against element e ^ j, j < 64, in the merge of runs of length k
__device__ inline unsigned rcs_step(unsigned v, int e, int k, int j) {
    const unsigned o = __shfl_xor(v, j);
    return ((e & j) == 0) == ((e & k) == 0) ? min(v, o) : max(v, o);
}

__device__ inline int rcs_sort_form(unsigned *key, int *ids, int n, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    int P = 64;
    while (P < n) P <<= 1;
    for (int e = tid; e < P; e += RCS_THREADS) key[e] = e < n ? (unsigned)ids[e] : RCS_PAD;
    __syncthreads();
    // runs of up to 64: the whole network in registers (P is a multiple of 64: a wave is in or out as one)
    for (int e = tid; e < P; e += RCS_THREADS) {
        unsigned v = key[e];
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) v = rcs_step(v, e, k, j);
        key[e] = v;
    }
    for (int k = 128; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            __syncthreads();
            for (int p = tid; p < (P >> 1); p += RCS_THREADS) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));   // pair p: elements i and i + j
                const unsigned a = key[i], b = key[i + j];
                if ((a > b) == ((i & k) == 0)) { key[i] = b; key[i + j] = a; }
            }
        }
        __syncthreads();
        for (int e = tid; e < P; e += RCS_THREADS) {
            unsigned v = key[e];
            for (int j = 32; j > 0; j >>= 1) v = rcs_step(v, e, k, j);
            key[e] = v;
        }
    }
    __syncthreads();
    // heads: the first of every run of equal ids
    int c0, c1;
    rcs_quarter(P >> 6, wave, c0, c1);
    int total = 0;
    for (int c = c0; c < c1; c++) {
        const int e = (c << 6) + lane;
        const unsigned v = key[e];
        total += __popcll(__ballot(v != RCS_PAD && (e == 0 || key[e - 1] != v)));
    }
    int off, all;
    rcs_exchange(key, total, tid, off, all);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = c0; c < c1; c++) {
        const int e = (c << 6) + lane;
        const unsigned v = key[e];
        const bool head = v != RCS_PAD && (e == 0 || key[e - 1] != v);
        const unsigned long long b = __ballot(head);
        if (head) ids[off + __popcll(b & below)] = (int)v;
        off += __popcll(b);
    }
    return all;
}

__device__ inline int rcs_bitmap_form(unsigned *bits, int *ids, int n, int W, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    for (int w = tid; w < W; w += RCS_THREADS) bits[w] = 0u;
    __syncthreads();
    for (int e = tid; e < n; e += RCS_THREADS) {
        const unsigned id = (unsigned)ids[e];
        atomicOr(&bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
    int c0, c1;
    rcs_quarter((W + 63) >> 6, wave, c0, c1);
    int total = 0;
    for (int c = c0; c < c1; c++) {
        const int w = (c << 6) + lane;
        total += w < W ? __popc(bits[w]) : 0;
    }
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    int off, all;
    rcs_exchange(bits, total, tid, off, all);
    for (int c = c0; c < c1; c++) {
        const int w = (c << 6) + lane;
        unsigned m = w < W ? bits[w] : 0u;
        const int cnt = __popc(m);
        int upto = cnt;   // inclusive prefix of the round's counts over the lanes
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(upto, d);
            upto += lane >= d ? y : 0;
        }
        int o = off + upto - cnt;
        for (; m; m &= m - 1u) ids[o++] = (w << 5) + __ffs((int)m) - 1;
        off += __shfl(upto, 63);
    }
    return all;
}

__global__ __launch_bounds__(RCS_THREADS) void k_rank_cand_sets(const RankCandSetsDev D) {
    extern __shared__ unsigned rcs_lds[];
    const int sec = blockIdx.x, tid = threadIdx.x;
    const int r0 = D.sec_r0[sec], n = D.sec_r0[sec + 1] - r0;
    if (n <= 0) {   // the whole workgroup: nothing else is touched
        if (tid == 0) D.set_size[sec] = 0;
        return;
    }
    const int size = D.sec_form[sec] == 2 ? rcs_bitmap_form(rcs_lds, D.raw + r0, n, (int)((D.num_item + 31u) >> 5), tid)
                                          : rcs_sort_form(rcs_lds, D.raw + r0, n, tid);
    if (tid == 0) D.set_size[sec] = size;
}

__global__ __launch_bounds__(RCS_THREADS) void k_rank_cand_pack(const RankCandSetsDev D) {
    const int sec = blockIdx.x * (RCS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (sec >= D.nsec) return;
    const int q0 = D.sec_q0[sec], nq = D.sec_q0[sec + 1] - q0;
    const int *set = D.raw + D.sec_r0[sec];
    for (int i = lane; i < nq; i += 64) D.cand_id[q0 + i] = set[i];
    if (!D.sec_p0) return;
    for (int p = D.sec_p0[sec] + lane; p < D.sec_p0[sec + 1]; p += 64) {
        const unsigned id = (unsigned)D.pos_id[p];
        int lo = 0, hi = nq;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)set[mid] < id) lo = mid + 1; else hi = mid;
        }
        const bool found = lo < nq && (unsigned)set[lo] == id;
        D.pos_at[p] = found ? q0 + lo : 0;
        if (!found) D.flag[0] = 1;
    }
}

int rank_cand_sets_lds_words(int64_t n, int64_t num_item, int form) {
    if (form == 2) return (int)std::max<int64_t>(4, (num_item + 31) / 32);   // (rcs_exchange borrows four words)
    int P = 64;
    while (P < n) P <<= 1;
    return P;
}

void launch_rank_cand_sets(const RankCandSetsDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    hipLaunchKernelGGL(k_rank_cand_sets, dim3((unsigned)D.nsec), dim3(RCS_THREADS), 4 * (size_t)D.lds_words, st, D);
}

void launch_rank_cand_pack(const RankCandSetsDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    hipLaunchKernelGGL(k_rank_cand_pack, dim3((unsigned)((D.nsec + RCS_THREADS / 64 - 1) / (RCS_THREADS / 64))), dim3(RCS_THREADS), 0, st, D);
}

}  // namespace svdf

// svdf_k_ranknegs.hip -- the negatives of sampled-negative ranking, drawn on the device: a wave per section writes
// the section's slice of cand_id -- its positives, then the first num_neg ids of the section's draw sequence (svdf_ranknegs_lists.h; the
// rule is stated in include/svdfeature_amd.h) that are neither excluded nor drawn before, in the order of the sequence -- where the score
// and count kernels of svdf_k_rankcand.hip read it.  The result is the sequential definition's for every input: round r evaluates the 64
// draws 64 r .. 64 r + 63 at once, one per lane, and accepts them in lane order.  Integer arithmetic only; a section belongs to one wave: no
// atomics, nothing depends on timing.
#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_ranknegs_lists.h"

namespace svdf {

// the slot a probe for `id` starts at: the top bits of a Fibonacci hash, `shift` = 32 - log2(slots)
__device__ __forceinline__ unsigned ng_slot(unsigned id, int shift) { return (id * 2654435761u) >> shift; }

__global__ __launch_bounds__(64) void k_rank_negs_draw(const RankNegsDev D) {
    extern __shared__ int ng_seen[];   // [D.slots] open addressing, linear probing; -1: free.  At most half full: a probe always ends
    const int sec = blockIdx.x, lane = threadIdx.x;
    const int p0 = D.sec_p0[sec], npos = D.sec_p0[sec + 1] - p0;
    int *row = D.neg_out ? D.neg_out + (size_t)sec * (size_t)D.num_neg : nullptr;
    if (npos == 0) {   // wave-uniform: nothing of a section without positives is drawn or scored
        if (row)
            for (int j = lane; j < D.num_neg; j += 64) row[j] = -1;
        return;
    }
    int *ids = D.cand_id + D.sec_q0[sec];
    for (int j = lane; j < npos; j += 64) ids[j] = D.pos_id[p0 + j];
    ids += npos;
    for (int j = lane; j < D.slots; j += 64) ng_seen[j] = -1;
    tn_wave_sync();
    const int *ex = D.ex_id + D.ex_p0[sec];
    const int nex = D.ex_p0[sec + 1] - D.ex_p0[sec];
    const uint64_t stream = rank_negs_stream(D.seed, (uint64_t)(D.sec0 + sec));
    const unsigned mask = (unsigned)D.slots - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    int have = 0;
    for (uint64_t t0 = 0; have < D.num_neg; t0 += 64) {   // `have` is wave-uniform
        const unsigned id = rank_negs_draw(stream, t0 + (uint64_t)lane, D.num_item);
        int lo = 0, hi = nex;   // excluded: binary search in the section's sorted list
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if ((unsigned)ex[m] < id) lo = m + 1; else hi = m;
        }
        bool ok = !(lo < nex && (unsigned)ex[lo] == id);
        if (ok)             // drawn in an earlier round
            for (unsigned h = ng_slot(id, D.shift);; h = (h + 1u) & mask) {
                const int v = ng_seen[h];
                if (v < 0) break;
                if ((unsigned)v == id) { ok = false; break; }
            }
        // drawn earlier in this round: in draw order, every candidate lane tells its id to the lanes above it
        for (unsigned long long m = __ballot(ok); m; m &= m - 1ull) {
            const int b = __ffsll(m) - 1;
            const unsigned other = (unsigned)__shfl((int)id, b);
            if (lane > b && id == other) ok = false;
        }
        const unsigned long long acc = __ballot(ok);
        const int at = have + __popcll(acc & below);
        const bool take = ok && at < D.num_neg;   // cut at the number still missing
        if (take) {
            ids[at] = (int)id;
            if (row) row[at] = (int)id;
        }
        const unsigned long long taken = __ballot(take);
        for (unsigned long long m = taken; m; m &= m - 1ull) {   // one insertion at a time, the same for the whole wave
            const unsigned nid = (unsigned)__shfl((int)id, __ffsll(m) - 1);
            if (lane == 0) {
                unsigned h = ng_slot(nid, D.shift);
                while (ng_seen[h] >= 0) h = (h + 1u) & mask;
                ng_seen[h] = (int)nid;
            }
        }
        have += __popcll(taken);
        tn_wave_sync();
    }
}

void launch_rank_negs(const RankNegsDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    hipLaunchKernelGGL(k_rank_negs_draw, dim3((unsigned)D.nsec), dim3(64), (size_t)D.slots * sizeof(int), st, D);
}

}  // namespace svdf

// svdf_k_ranktopn_mfma.hip -- the selecting sweep of the top-N calls on the matrix cores, the opt-in second scoring
// mode of svdf_rank_topn* / svdf_item_topn (knob rank_topn_scores = 1).  Same RankTopnDev, same keys, lists, ban masks, NaN flag and merge
// as the pinned sweep (svdf_k_ranktopn.hip); what differs is the dot, which is mx_sweep's (svdf_k_rankmfma.h: the tiling, the K order, the
// stage, the ban masks, the bias add and the output layout are stated there, once for this kernel and the counting sweep of section 6aj).
// A row of that loop is a section here: the workgroup owns the sections 64 blockIdx.x .. + 63.
//
// Selection.  Handed a tile in the MFMA's own output layout, a lane compares each live key with its section's threshold in LDS.  One ballot
// ends the tile for the wave when no lane has a hit -- the common case once the lists hold top_n keys.  Otherwise the wave walks its
// sections that have hits, and appends per section through ballot prefixes, tn_select's logic with a step of 128 candidates.
#include <cstdlib>

#include "svdf_k_rankmfma.h"

namespace svdf {

// DEEP (section 6al): a list that cannot take a tile is cut where it lies by tn_select_keep; a wave's scratch is its histogram.
template <bool DEEP>
__global__ __launch_bounds__(256) void k_rank_topn_sweep_mfma(const DevParams P, const RankTopnDev D) {
    __shared__ MxLds L;
    __shared__ tn_key_t l_scr[4][tn_scratch_keys(DEEP)];
    __shared__ tn_key_t l_thr[MX_TS];
    __shared__ int l_cnt[MX_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;
    const int sec_base = blockIdx.x * MX_TS;
    const int nrows = D.nsec - sec_base < MX_TS ? D.nsec - sec_base : MX_TS;
    for (int q = tid; q < MX_TS; q += 256) { l_thr[q] = 0ull; l_cnt[q] = 0; }   // read behind mx_sweep's first barrier

    mx_sweep(P, D.user_rows, D.sec_user, D.item_rows, D.item_bias, D.ban_p0, D.ban_item, D.items_per_block, nrows, L,
             [&](int row) { return sec_base + row; },
             [&](long it0, int sec0, const mx_f4 *acc, unsigned live) {
        tn_key_t key[MX_NB][4];
        unsigned hit = 0u;   // bit 4 b + r
        tn_key_t thr4[4];
#pragma unroll
        for (int r = 0; r < 4; r++) thr4[r] = l_thr[sec0 + r];
#pragma unroll
        for (int b = 0; b < MX_NB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                key[b][r] = tn_key(acc[b][r], (int)(it0 + 16 * b + lcol));
                if (((live >> (4 * b + r)) & 1u) && key[b][r] > thr4[r]) hit |= 1u << (4 * b + r);   // a NaN is never listed (it flags the section)
            }
        }
        if (__ballot(hit != 0u)) {
            const tn_key_t below = (1ull << lane) - 1ull;
            tn_key_t *scratch = l_scr[wave];
            for (int gq = 0; gq < 4; gq++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const bool mine = lgrp == gq;
                    if (!__ballot(mine && (hit & (0x11111111u << r)))) continue;   // wave-uniform
                    const int sec = wave * 16 + 4 * gq + r;
                    tn_key_t *list = D.list + ((size_t)(sec_base + sec) * D.gy + blockIdx.y) * D.cap;
                    int cnt = __builtin_amdgcn_readfirstlane(l_cnt[sec]);
                    tn_key_t thr = l_thr[sec];
                    if (cnt + MX_TI > D.cap) {   // no room for a whole step: cut to the top_n largest, which raises the threshold
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's own appends, by other lanes, are read back
                        if constexpr (DEEP) {
                            cnt = tn_select_keep(list, cnt, D.top_n, lane, reinterpret_cast<int *>(scratch), thr);
                        } else {
                            for (int i = lane; i < cnt; i += 64) scratch[i] = list[i];
                            cnt = tn_sort_keep(scratch, cnt, D.top_n, lane, thr);
                            for (int i = lane; i < cnt; i += 64) list[i] = scratch[i];
                        }
                        if (lane == 0) l_thr[sec] = thr;
                        tn_wave_sync();
                    }
#pragma unroll
                    for (int b = 0; b < MX_NB; b++) {
                        const bool take = mine && ((hit >> (4 * b + r)) & 1u) && key[b][r] > thr;
                        const tn_key_t bl = __ballot(take);
                        if (take) list[cnt + __popcll(bl & below)] = key[b][r];   // cnt + popc <= cap
                        cnt += __popcll(bl);
                    }
                    if (lane == 0) l_cnt[sec] = cnt;
                    tn_wave_sync();
                }
            }
        }
    });
    for (int q = tid; q < nrows; q += 256) {
        D.list_cnt[(size_t)(sec_base + q) * D.gy + blockIdx.y] = l_cnt[q];
        if (L.nan[q]) atomicAdd(&D.nan_cnt[sec_base + q], L.nan[q]);
    }
}


void launch_rank_topn_sweep_mfma(const DevParams &P, const RankTopnDev &D, hipStream_t st) {
    // a list takes top_n kept keys and one tile's appends, and a wave's sort buffer a whole list: rank_topn_cap(.., matrix = 1) says so;
    // a launch with another capacity would write past a list
    // (a deep list is cut in place, so only the workspace bounds it: rank_topn_deep_cap)
    if (D.nsec <= 0 || D.cap < D.top_n + MX_TI || D.cap > (D.deep ? RANK_TOPN_DEEP_MAX_CAP : TN_SORT)) abort();
    const dim3 grid((unsigned)((D.nsec + MX_TS - 1) / MX_TS), (unsigned)D.gy);
    if (D.deep) hipLaunchKernelGGL(k_rank_topn_sweep_mfma<true>, grid, dim3(256), 0, st, P, D);
    else hipLaunchKernelGGL(k_rank_topn_sweep_mfma<false>, grid, dim3(256), 0, st, P, D);
}

}  // namespace svdf

// svdf_k_ranktopn_mfma.hip -- the selecting sweep of the top-N calls on the matrix cores, the opt-in second scoring
// mode of svdf_rank_topn* / svdf_item_topn (knob rank_topn_scores = 1).  Same RankTopnDev, same keys, lists, ban masks, NaN flag and merge
// as the pinned sweep (svdf_k_ranktopn.hip); what differs is the dot: v_mfma_f32_16x16x4_f32, fp32 in, fp32 accumulate, ONE accumulator
// per score, K walked in ascending chunks of 32 floats through LDS at every row width (1 .. 1024 floats).
//
// Tiling.  A workgroup (4 waves) owns the sections 64 blockIdx.x .. + 63 and the item range blockIdx.y, which it walks in tiles of 128
// items.  Wave w owns the sections 16 w .. 16 w + 15 against all 128 items of the tile: 8 MFMA blocks of 16 x 16, 32 accumulator registers,
// the A operand (user side) read once per K step and reused across the 8 blocks.  A STEP of the flat loop is one (item tile, K chunk):
// 64 user rows and 128 item rows of 32 floats each, row-major with a pitch of 36 floats (float4 reads of 16 consecutive lanes then touch
// every bank once), double-buffered -- the global loads of step t + 1 are in flight while the MFMAs of step t run, one barrier per step.
// Pad floats (k .. chunk end) and rows past the sections / the item range are staged as zeros, never trusted, the latter never read.
//
// K order.  Inside a group of 16 floats MFMA j (0 .. 3) multiplies the elements {j, 4 + j, 8 + j, 12 + j}: lane l supplies the float4 at
// 4 (l / 16) of its row, one component per MFMA, so one ds_read_b128 feeds four MFMAs.  Both operands use the same map, so the products
// pair up; the order is a function of the element index alone, hence a score's bits of its two rows, the bias and k alone.
//
// Selection.  After the last chunk of a tile lane l holds, in register r of block b, the dot of section 4 (l / 16) + r of its wave and item
// 16 b + l % 16 of the tile -- the MFMA's own output layout; nothing is transposed.  The lane adds the bias, clears banned and out-of-range
// pairs from the section's mask words, counts NaNs and compares each key with its section's threshold in LDS.  One ballot ends the tile
// for the wave when no lane has a hit -- the common case once the lists hold top_n keys.  Otherwise the wave walks its sections that have
// hits, and appends per section through ballot prefixes, tn_select's logic with a step of 128 candidates.
#include <cstdlib>

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

typedef float tm_f4 __attribute__((ext_vector_type(4)));

constexpr int TM_TS = 64;                 // sections of a workgroup (TN_TS of the pinned sweep)
constexpr int TM_TI = RANK_TOPN_MATRIX_TILE;   // items of a tile: 8 MFMA blocks per wave
constexpr int TM_NB = TM_TI / 16;         // MFMA blocks of a wave
constexpr int TM_KC = 32;                 // floats of a K chunk
constexpr int TM_LP = TM_KC + 4;          // floats between two rows of a stage in LDS
constexpr int TM_ROWS = TM_TS + TM_TI;    // rows of a stage: user rows, then item rows
constexpr int TM_LD = TM_ROWS * (TM_KC / 4) / 256;   // float4 loads of a thread per step
constexpr int TM_LU = TM_TS * (TM_KC / 4) / 256;     // ... the first of which are user rows

// first entry >= x of the ascending ids ban[b0 .. b1)
__device__ __forceinline__ int tm_lower_bound(const int *__restrict__ ban, int b0, int b1, long x) {
    while (b0 < b1) {
        const int m = b0 + ((b1 - b0) >> 1);
        if ((long)ban[m] < x) b0 = m + 1; else b1 = m;
    }
    return b0;
}

__device__ __forceinline__ float4 tm_clip(float4 v, int e0, int k) {   // elements e0 .. e0 + 3 of a row: those at k and beyond are pads
    if (e0 + 3 >= k) {
        if (e0 >= k) v.x = 0.0f;
        if (e0 + 1 >= k) v.y = 0.0f;
        if (e0 + 2 >= k) v.z = 0.0f;
        v.w = 0.0f;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_rank_topn_sweep_mfma(const DevParams P, const RankTopnDev D) {
    __shared__ __attribute__((aligned(16))) float l_stage[2][TM_ROWS * TM_LP];
    __shared__ tn_key_t l_scr[4][TN_SORT];
    __shared__ tn_key_t l_thr[TM_TS];
    __shared__ tn_key_t l_mask[2][TM_TS][TM_TI / 64];   // the ban bits of tile t in [t & 1], built one tile ahead
    __shared__ int l_cnt[TM_TS];
    __shared__ int l_nan[TM_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;   // MFMA operand row / output column, and K quarter / output row group
    const int sec_base = blockIdx.x * TM_TS;
    const int nrows = D.nsec - sec_base < TM_TS ? D.nsec - sec_base : TM_TS;
    const int k = P.k, nq = P.pitch >> 2;           // float4s of a row in memory
    const int nch = (k + TM_KC - 1) / TM_KC;
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    const long i_begin = (long)blockIdx.y * D.items_per_block;
    const long i_end = i_begin + D.items_per_block < (long)P.num_item ? i_begin + D.items_per_block : (long)P.num_item;
    const long ntile = i_end > i_begin ? (i_end - i_begin + TM_TI - 1) / TM_TI : 0;
    const long nstep = ntile * nch;

    // what this thread stages every step: TM_LD (row, float4) slots of the 192 x 8 of a stage; user slots keep their row pointer
    const float4 *urow[TM_LU];
#pragma unroll
    for (int i = 0; i < TM_LU; i++) {
        const int row = (tid + 256 * i) >> 3;
        urow[i] = nullptr;
        if (row < nrows) urow[i] = re_section_row(P, D.user_rows, D.sec_user, sec_base + row);
    }
    for (int q = tid; q < TM_TS; q += 256) { l_thr[q] = 0ull; l_cnt[q] = 0; l_nan[q] = 0; }
    int bcur = 0, bend = 0;   // thread t < nrows: what is left of section t's ban list
    if (tid < nrows) {
        bend = D.ban_p0[sec_base + tid + 1];
        bcur = tm_lower_bound(D.ban_item, D.ban_p0[sec_base + tid], bend, i_begin);
    }

    float4 g[TM_LD];
    auto fetch = [&](long step) {   // the global loads of one step into registers
        const long tile = step / nch;
        const int c = (int)(step - tile * nch);
        const long it0 = i_begin + tile * TM_TI;
#pragma unroll
        for (int i = 0; i < TM_LD; i++) {
            const int slot = tid + 256 * i, row = slot >> 3, q = c * (TM_KC / 4) + (slot & 7);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q < nq) {
                if (i < TM_LU) {
                    if (urow[i]) v = urow[i][q];
                } else if (it0 + (row - TM_TS) < i_end) {
                    v = re_item_row(ibase, P.pitch, it0 + (row - TM_TS))[q];
                }
                v = tm_clip(v, 4 * q, k);
            }
            g[i] = v;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < TM_LD; i++) {
            const int slot = tid + 256 * i;
            *reinterpret_cast<float4 *>(&l_stage[buf][(slot >> 3) * TM_LP + 4 * (slot & 7)]) = g[i];
        }
    };

    auto ban_bits = [&](long tile) {   // thread t < 64: section t's banned items of one tile, from its cursor
        if (tid < TM_TS) {
            const long it0 = i_begin + tile * TM_TI;
            tn_key_t m[TM_TI / 64];
#pragma unroll
            for (int w = 0; w < TM_TI / 64; w++) m[w] = 0ull;
            while (bcur < bend) {
                const long d = (long)D.ban_item[bcur] - it0;   // >= 0: the cursor has passed everything below it0
                if (d >= TM_TI) break;
#pragma unroll
                for (int w = 0; w < TM_TI / 64; w++)
                    if ((int)(d >> 6) == w) m[w] |= 1ull << (d & 63);
                bcur++;
            }
#pragma unroll
            for (int w = 0; w < TM_TI / 64; w++) l_mask[tile & 1][tid][w] = m[w];
        }
    };

    tm_f4 acc[TM_NB];
    if (nstep > 0) { fetch(0); stash(0); ban_bits(0); }
    __syncthreads();
    for (long step = 0; step < nstep; step++) {
        const int buf = (int)(step & 1);
        const long tile = step / nch;
        const int c = (int)(step - tile * nch);
        const long it0 = i_begin + tile * TM_TI;
        if (step + 1 < nstep) fetch(step + 1);
        if (c == 0) {
#pragma unroll
            for (int b = 0; b < TM_NB; b++) acc[b] = (tm_f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (tile + 1 < ntile) ban_bits(tile + 1);   // read behind the barrier of this step at the earliest
        }
        if (wave * 16 < nrows) {   // wave-uniform: a wave without sections only stages
            const float *su = &l_stage[buf][(wave * 16 + lcol) * TM_LP + 4 * lgrp];
            const float *si = &l_stage[buf][(TM_TS + lcol) * TM_LP + 4 * lgrp];
            const int ng = k - c * TM_KC > 16 ? 2 : 1;   // groups of 16 floats of this chunk that hold elements below k
            for (int h = 0; h < ng; h++) {
                const float4 a = *reinterpret_cast<const float4 *>(su + 16 * h);
                float4 bv[TM_NB];
#pragma unroll
                for (int b = 0; b < TM_NB; b++) bv[b] = *reinterpret_cast<const float4 *>(si + 16 * b * TM_LP + 16 * h);
#pragma unroll
                for (int b = 0; b < TM_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[b].x, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < TM_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[b].y, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < TM_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv[b].z, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < TM_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv[b].w, acc[b], 0, 0, 0);
            }
        }
        if (c == nch - 1 && wave * 16 < nrows) {
            // ---- the tile's scores are complete: register r of block b is (section wave * 16 + 4 lgrp + r, item it0 + 16 b + lcol)
            const int sec0 = wave * 16 + 4 * lgrp;
            tn_key_t key[TM_NB][4];
            unsigned hit = 0u, nanb = 0u;   // bit 4 b + r
            tn_key_t thr4[4], mk[4][TM_TI / 64];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                thr4[r] = l_thr[sec0 + r];
#pragma unroll
                for (int w = 0; w < TM_TI / 64; w++) mk[r][w] = l_mask[tile & 1][sec0 + r][w];
            }
#pragma unroll
            for (int b = 0; b < TM_NB; b++) {
                const long cnd = it0 + 16 * b + lcol;
                const bool in = cnd < i_end;
                const float bias = in ? ibias[cnd] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float s = acc[b][r] + bias;
                    const bool ranked = in && sec0 + r < nrows && !((mk[r][b >> 2] >> (16 * (b & 3) + lcol)) & 1ull);
                    key[b][r] = tn_key(s, (int)cnd);
                    if (ranked && s != s) nanb |= 1u << (4 * b + r);
                    if (ranked && s == s && key[b][r] > thr4[r]) hit |= 1u << (4 * b + r);   // a NaN is never listed (it flags the section)
                }
            }
            if (__ballot(nanb != 0u)) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int nn = __popc(nanb & (0x11111111u << r));
                    if (nn) atomicAdd(&l_nan[sec0 + r], nn);
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
                        if (cnt + TM_TI > D.cap) {   // no room for a whole step: cut to the top_n largest, which raises the threshold
                            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's own appends, by other lanes, are read back
                            for (int i = lane; i < cnt; i += 64) scratch[i] = list[i];
                            cnt = tn_sort_keep(scratch, cnt, D.top_n, lane, thr);
                            for (int i = lane; i < cnt; i += 64) list[i] = scratch[i];
                            if (lane == 0) l_thr[sec] = thr;
                            tn_wave_sync();
                        }
#pragma unroll
                        for (int b = 0; b < TM_NB; b++) {
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
        }
        if (step + 1 < nstep) stash(buf ^ 1);   // the other stage: every wave left it at the previous barrier
        __syncthreads();
    }
    __syncthreads();
    for (int q = tid; q < nrows; q += 256) {
        D.list_cnt[(size_t)(sec_base + q) * D.gy + blockIdx.y] = l_cnt[q];
        if (l_nan[q]) atomicAdd(&D.nan_cnt[sec_base + q], l_nan[q]);
    }
}

void launch_rank_topn_sweep_mfma(const DevParams &P, const RankTopnDev &D, hipStream_t st) {
    // a list takes top_n kept keys and one tile's appends, and a wave's sort buffer a whole list: rank_topn_cap(.., matrix = 1) says so;
    // a launch with another capacity would write past a list
    if (D.nsec <= 0 || D.cap < D.top_n + TM_TI || D.cap > TN_SORT) abort();
    const dim3 grid((unsigned)((D.nsec + TM_TS - 1) / TM_TS), (unsigned)D.gy);
    hipLaunchKernelGGL(k_rank_topn_sweep_mfma, grid, dim3(256), 0, st, P, D);
}

}  // namespace svdf

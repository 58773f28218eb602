// svdf_k_rankmfma.h -- the scoring loop of the sweeps on the matrix cores: k_rank_topn_sweep_mfma (svdf_k_ranktopn_mfma.hip, DESIGN.md section
// 6ah) and k_rank_eval_sweep_mfma (svdf_k_rankeval_mfma.hip, section 6aj) both call mx_sweep, so "the approximate score" that Delta_s of
// section 6ai bounds has this one statement.  v_mfma_f32_16x16x4_f32, fp32 in, fp32 accumulate, ONE accumulator per score, K walked in
// ascending chunks of 32 floats through LDS at every row width (1 .. 1024 floats).
//
// Tiling.  A workgroup (4 waves) owns 64 rows (a row scores with the user row of one section) and the item range blockIdx.y, which it walks
// in tiles of 128 items.  Wave w owns the rows 16 w .. 16 w + 15 against all 128 items of the tile: 8 MFMA blocks of 16 x 16, 32 accumulator
// registers, the A operand (user side) read once per K step and reused across the 8 blocks.  A STEP of the flat loop is one (item tile, K
// chunk): 64 user rows and 128 item rows of 32 floats each, row-major with a pitch of 36 floats (float4 reads of 16 consecutive lanes then
// touch every bank once), double-buffered -- the global loads of step t + 1 are in flight while the MFMAs of step t run, one barrier per
// step.  Pad floats (k .. chunk end) and rows past the last row / the item range are staged as zeros, never trusted, the latter never read.
//
// K order.  Inside a group of 16 floats MFMA j (0 .. 3) multiplies the elements {j, 4 + j, 8 + j, 12 + j}: lane l supplies the float4 at
// 4 (l / 16) of its row, one component per MFMA, so one ds_read_b128 feeds four MFMAs.  Both operands use the same map, so the products
// pair up; the order is a function of the element index alone, hence a score's bits of its two rows, the bias and k alone.
//
// Output.  After the last chunk of a tile lane l holds, in register r of block b, the dot of row 4 (l / 16) + r of its wave and item
// 16 b + l % 16 of the tile -- the MFMA's own output layout; nothing is transposed.  The lane adds the bias, drops banned and out-of-range
// pairs by the row's mask words (built one tile ahead from the ascending ban cursor of the row's section), counts NaNs into L.nan, and hands
// the tile to the caller: on_tile(it0, row0, acc, live) with acc[b][r] the score (bias added) of (row row0 + r, item it0 + 16 b + lcol) and
// bit 4 b + r of `live` set where that pair is ranked and its score is no NaN.  Only waves that own a row call it, wave-uniformly.
#pragma once

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

typedef float mx_f4 __attribute__((ext_vector_type(4)));

constexpr int MX_TS = 64;                 // rows of a workgroup (TN_TS of the pinned sweep)
constexpr int MX_TI = RANK_TOPN_MATRIX_TILE;   // items of a tile: 8 MFMA blocks per wave
constexpr int MX_NB = MX_TI / 16;         // MFMA blocks of a wave
constexpr int MX_KC = 32;                 // floats of a K chunk
constexpr int MX_LP = MX_KC + 4;          // floats between two rows of a stage in LDS
constexpr int MX_ROWS = MX_TS + MX_TI;    // rows of a stage: user rows, then item rows
constexpr int MX_LD = MX_ROWS * (MX_KC / 4) / 256;   // float4 loads of a thread per step
constexpr int MX_LU = MX_TS * (MX_KC / 4) / 256;     // ... the first of which are user rows

struct MxLds {   // what mx_sweep keeps in LDS; the caller declares one __shared__
    __attribute__((aligned(16))) float stage[2][MX_ROWS * MX_LP];
    tn_key_t mask[2][MX_TS][MX_TI / 64];   // the ban bits of tile t in [t & 1], built one tile ahead
    int nan[MX_TS];                        // ranked candidates of a row with a NaN score, over the whole item range
};

// first entry >= x of the ascending ids ban[b0 .. b1)
__device__ __forceinline__ int mx_lower_bound(const int *__restrict__ ban, int b0, int b1, long x) {
    while (b0 < b1) {
        const int m = b0 + ((b1 - b0) >> 1);
        if ((long)ban[m] < x) b0 = m + 1; else b1 = m;
    }
    return b0;
}

__device__ __forceinline__ float4 mx_clip(float4 v, int e0, int k) {   // elements e0 .. e0 + 3 of a row: those at k and beyond are pads
    if (e0 + 3 >= k) {
        if (e0 >= k) v.x = 0.0f;
        if (e0 + 1 >= k) v.y = 0.0f;
        if (e0 + 2 >= k) v.z = 0.0f;
        v.w = 0.0f;
    }
    return v;
}

// The sweep of one workgroup (256 threads) over its item range.  nrows (<= 64) rows are live; sec_of(row) is the section of a live row, whose
// user row and ban list ban_item[ban_p0[sec] .. ban_p0[sec + 1]) the row scores with.  Ends behind a barrier: L.nan is complete.
template <class SecOf, class OnTile>
__device__ __forceinline__ void mx_sweep(const DevParams &P, const float *user_rows, const unsigned *sec_user, const float *item_rows,
                                         const float *item_bias, const int *ban_p0, const int *ban_item, long items_per_block, int nrows, MxLds &L,
                                         SecOf sec_of, OnTile on_tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;   // MFMA operand row / output column, and K quarter / output row group
    const int k = P.k, nq = P.pitch >> 2;           // float4s of a row in memory
    const int nch = (k + MX_KC - 1) / MX_KC;
    const float *ibase = re_item_base(P, item_rows), *ibias = re_item_bias(P, item_bias);
    const long i_begin = (long)blockIdx.y * items_per_block;
    const long i_end = i_begin + items_per_block < (long)P.num_item ? i_begin + items_per_block : (long)P.num_item;
    const long ntile = i_end > i_begin ? (i_end - i_begin + MX_TI - 1) / MX_TI : 0;
    const long nstep = ntile * nch;

    // what this thread stages every step: MX_LD (row, float4) slots of the 192 x 8 of a stage; user slots keep their row pointer
    const float4 *urow[MX_LU];
#pragma unroll
    for (int i = 0; i < MX_LU; i++) {
        const int row = (tid + 256 * i) >> 3;
        urow[i] = nullptr;
        if (row < nrows) urow[i] = re_section_row(P, user_rows, sec_user, sec_of(row));
    }
    for (int q = tid; q < MX_TS; q += 256) L.nan[q] = 0;
    int bcur = 0, bend = 0;   // thread t < nrows: what is left of the ban list of row t's section
    if (tid < nrows) {
        const int sec = sec_of(tid);
        bend = ban_p0[sec + 1];
        bcur = mx_lower_bound(ban_item, ban_p0[sec], bend, i_begin);
    }

    float4 g[MX_LD];
    auto fetch = [&](long step) {   // the global loads of one step into registers
        const long tile = step / nch;
        const int c = (int)(step - tile * nch);
        const long it0 = i_begin + tile * MX_TI;
#pragma unroll
        for (int i = 0; i < MX_LD; i++) {
            const int slot = tid + 256 * i, row = slot >> 3, q = c * (MX_KC / 4) + (slot & 7);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (q < nq) {
                if (i < MX_LU) {
                    if (urow[i]) v = urow[i][q];
                } else if (it0 + (row - MX_TS) < i_end) {
                    v = re_item_row(ibase, P.pitch, it0 + (row - MX_TS))[q];
                }
                v = mx_clip(v, 4 * q, k);
            }
            g[i] = v;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < MX_LD; i++) {
            const int slot = tid + 256 * i;
            *reinterpret_cast<float4 *>(&L.stage[buf][(slot >> 3) * MX_LP + 4 * (slot & 7)]) = g[i];
        }
    };
    auto ban_bits = [&](long tile) {   // thread t < 64: the banned items of row t's section in one tile, from its cursor
        if (tid < MX_TS) {
            const long it0 = i_begin + tile * MX_TI;
            tn_key_t m[MX_TI / 64];
#pragma unroll
            for (int w = 0; w < MX_TI / 64; w++) m[w] = 0ull;
            while (bcur < bend) {
                const long d = (long)ban_item[bcur] - it0;   // >= 0: the cursor has passed everything below it0
                if (d >= MX_TI) break;
#pragma unroll
                for (int w = 0; w < MX_TI / 64; w++)
                    if ((int)(d >> 6) == w) m[w] |= 1ull << (d & 63);
                bcur++;
            }
#pragma unroll
            for (int w = 0; w < MX_TI / 64; w++) L.mask[tile & 1][tid][w] = m[w];
        }
    };

    mx_f4 acc[MX_NB];
    if (nstep > 0) { fetch(0); stash(0); ban_bits(0); }
    __syncthreads();
    for (long step = 0; step < nstep; step++) {
        const int buf = (int)(step & 1);
        const long tile = step / nch;
        const int c = (int)(step - tile * nch);
        const long it0 = i_begin + tile * MX_TI;
        if (step + 1 < nstep) fetch(step + 1);
        if (c == 0) {
#pragma unroll
            for (int b = 0; b < MX_NB; b++) acc[b] = (mx_f4){0.0f, 0.0f, 0.0f, 0.0f};
            if (tile + 1 < ntile) ban_bits(tile + 1);   // read behind the barrier of this step at the earliest
        }
        if (wave * 16 < nrows) {   // wave-uniform: a wave without rows only stages
            const float *su = &L.stage[buf][(wave * 16 + lcol) * MX_LP + 4 * lgrp];
            const float *si = &L.stage[buf][(MX_TS + lcol) * MX_LP + 4 * lgrp];
            const int ng = k - c * MX_KC > 16 ? 2 : 1;   // groups of 16 floats of this chunk that hold elements below k
            for (int h = 0; h < ng; h++) {
                const float4 a = *reinterpret_cast<const float4 *>(su + 16 * h);
                float4 bv[MX_NB];
#pragma unroll
                for (int b = 0; b < MX_NB; b++) bv[b] = *reinterpret_cast<const float4 *>(si + 16 * b * MX_LP + 16 * h);
#pragma unroll
                for (int b = 0; b < MX_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[b].x, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < MX_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[b].y, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < MX_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv[b].z, acc[b], 0, 0, 0);
#pragma unroll
                for (int b = 0; b < MX_NB; b++) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv[b].w, acc[b], 0, 0, 0);
            }
        }
        if (c == nch - 1 && wave * 16 < nrows) {
            // ---- the tile's scores are complete: register r of block b is (row wave * 16 + 4 lgrp + r, item it0 + 16 b + lcol)
            const int row0 = wave * 16 + 4 * lgrp;
            unsigned live = 0u, nanb = 0u;   // bit 4 b + r
            tn_key_t mk[4][MX_TI / 64];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int w = 0; w < MX_TI / 64; w++) mk[r][w] = L.mask[tile & 1][row0 + r][w];
#pragma unroll
            for (int b = 0; b < MX_NB; b++) {
                const long cnd = it0 + 16 * b + lcol;
                const bool in = cnd < i_end;
                const float bias = in ? ibias[cnd] : 0.0f;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float s = acc[b][r] + bias;
                    const bool ranked = in && row0 + r < nrows && !((mk[r][b >> 2] >> (16 * (b & 3) + lcol)) & 1ull);
                    acc[b][r] = s;   // the accumulators start from zero at the next tile
                    if (ranked && s != s) nanb |= 1u << (4 * b + r);
                    if (ranked && s == s) live |= 1u << (4 * b + r);
                }
            }
            if (__ballot(nanb != 0u)) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int nn = __popc(nanb & (0x11111111u << r));
                    if (nn) atomicAdd(&L.nan[row0 + r], nn);
                }
            }
            on_tile(it0, row0, acc, live);
        }
        if (step + 1 < nstep) stash(buf ^ 1);   // the other stage: every wave left it at the previous barrier
        __syncthreads();
    }
    __syncthreads();
}

}  // namespace svdf

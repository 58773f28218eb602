// svdf_k_foldin.hip -- fold-in on the live model (svdf_fold_in): per section the ridge least-squares row of one user
// against the fixed item side, p = (sum_j q_j q_j^T + reg I)^-1 sum_j y_j q_j.  gfx950 only.
//
// One workgroup owns a section for its whole life: the Gram matrix is summed in accumulator registers, written once to LDS, factorised and
// solved there, and only the row leaves the workgroup.  k_fold_in<NB> is templated on the width class NB = blocks of 16 columns, 1 / 2 / 4 /
// 8 (k <= 16 / 32 / 64 / 128); the narrow classes run one wave per workgroup, the wide ones four.
//
// Gram sum.  The reduction dimension of v_mfma_f32_16x16x4_f32 is the RATINGS.  A stage holds the item rows of 16 consecutive ratings,
// row-major with LP = 16 NB + 16 floats between rows (NB = 1: 16), so the 64 lanes of an operand read -- 16 consecutive columns of four
// consecutive ratings -- touch 64 different banks.  Columns k .. 16 NB - 1 and ratings past the section's end are staged as zeros.  BOTH
// operands of block (bi, bj) come from that stage: lane l supplies A[i = l % 16][r = l / 16] = q_r[16 bi + i] and B[r][j = l % 16] =
// q_r[16 bj + j], four MFMAs per block and stage.  Only the NB (NB + 1) / 2 blocks on and below the diagonal exist; block t belongs to wave
// t % W and sits in accumulator t / W (NB = 8: nine blocks, 36 registers a wave).  b = sum_j y_j q_j comes from the same stage by plain
// fmas, one column per thread.  The stage is double-buffered: the loads of chunk c + 1 (whose item ids were fetched one chunk earlier)
// are in flight while chunk c is multiplied; one barrier per chunk.
//
// Solve.  The blocks go to LDS once, column-major inside a block (the MFMA's output is four consecutive rows of one column per lane: one
// ds_write_b128), reg is added to the diagonal, and the matrix is factorised in place as L D L^T -- the Cholesky factorisation without
// its square roots, column by column, right-looking: after column j every thread updates its share of the trailing lower triangle,
// (i, c) -= v_ij v_cj / D_j.  Column j itself is left as v_ij = L_ij D_j and never rewritten, which is what lets a column take ONE barrier.
// b rides along as one more row of the matrix, so the forward substitution costs nothing of its own: after the last column it holds
// z = L^-1 b.  Only the k real rows and columns are walked; the pad columns of the last block are never read.  Wave 0 then substitutes
// backwards, x_i = (z_i - sum_{m > i} v_mi x_m) / D_i, column-oriented with z and x in registers (lane l: elements l and l + 64) and x_i
// handed round by v_readlane, without a barrier; it stores the row to rows_out and, with `write`, to W_user.
//
// LDS at NB = 8: 36 blocks x 1 KiB + 2 stages x 16 x 144 floats + b + y = 55 936 bytes.  No scratch in any instantiation.
#include <algorithm>

#include "svdf_kernels.h"

namespace svdf {

typedef float fi_f4 __attribute__((ext_vector_type(4)));

template <int NB>
struct FiShape {
    static constexpr int T = NB >= 4 ? 256 : 64;        // threads of a workgroup
    static constexpr int W = T / 64;                    // waves
    static constexpr int N = 16 * NB;                   // columns of the class
    static constexpr int LP = N + (NB == 1 ? 0 : 16);   // floats between two ratings of a stage
    static constexpr int NT = NB * (NB + 1) / 2;        // blocks on and below the diagonal
    static constexpr int NS = (NT + W - 1) / W;         // ... of one wave
    static constexpr int LD = 64 * NB / T;              // float4 loads of a thread per stage (16 ratings x 4 NB float4s)
    static constexpr int G = T / 16;                    // column groups of the trailing update: thread (li, g) owns rows == li (mod 16), columns == g (mod G)
    static constexpr int NC = N / G;                    // columns of a thread
    static constexpr int NE = (N + 63) / 64;            // elements of a lane in the backward substitution
};

template <int NB>
struct FiLds {
    __attribute__((aligned(16))) float stage[2][16 * FiShape<NB>::LP];
    __attribute__((aligned(16))) float tri[FiShape<NB>::NT * 256];   // block (bi, bj) at (bi (bi + 1) / 2 + bj) * 256, element (i, c) at 16 c + i
    float y[2][16];
    float b[FiShape<NB>::N];
};

__device__ __forceinline__ int fi_blk(int bi, int bj) { return ((bi * (bi + 1)) / 2 + bj) << 8; }
// element (i, c), i >= c, of the lower triangle
__device__ __forceinline__ int fi_at(int i, int c) { return fi_blk(i >> 4, c >> 4) + ((c & 15) << 4) + (i & 15); }

template <int NB>
__global__ __launch_bounds__(FiShape<NB>::T) void k_fold_in(const DevParams P, const FoldInDev D) {
    using S = FiShape<NB>;
    __shared__ FiLds<NB> L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 15, lgrp = lane >> 4;   // MFMA: operand row / output column, and K index / output row group
    const int li = tid & 15, g = tid >> 4;          // trailing update: row class, column class
    const int k = P.k, nq = P.pitch >> 2;
    const float *ibase = P.W + (size_t)P.item_off * P.pitch, *ibias = P.bias + P.item_off;

    // the blocks of this wave: t = wave + W i -> (bi, bj), bj <= bi
    int bi[S::NS], bj[S::NS];
#pragma unroll
    for (int i = 0; i < S::NS; i++) {
        const int t = wave + S::W * i;
        int r = 0;
        while (((r + 1) * (r + 2)) / 2 <= t) r++;
        bi[i] = r; bj[i] = t - (r * (r + 1)) / 2;
    }

    for (long sec = blockIdx.x; sec < D.nsec; sec += gridDim.x) {
        const unsigned u = D.user[sec];
        const long j0 = (long)D.ptr[sec], j1 = (long)D.ptr[sec + 1];
        float *out = D.rows_out + (size_t)sec * (size_t)k;
        float *wrow = P.W + (size_t)(P.user_off + u) * P.pitch;
        if (j1 == j0) {   // (uniform over the workgroup) no rating: the zero row
            for (int c = tid; c < k; c += S::T) {
                out[c] = 0.0f;
                if (D.write) wrow[c] = 0.0f;
            }
            continue;
        }
        const float lin = P.base_score + (P.no_user_bias ? 0.0f : P.bias[P.user_off + u]);
        const long nch = (j1 - j0 + 15) >> 4;

        // ---- the Gram sum
        unsigned idn[S::LD];   // the item of this thread's rating in the NEXT chunk to fetch
#pragma unroll
        for (int i = 0; i < S::LD; i++) {
            const long j = j0 + (tid + S::T * i) / (4 * NB);
            idn[i] = j < j1 ? D.item[j] : 0u;
        }
        float4 gq[S::LD];
        float gy[S::LD];
        auto fetch = [&](long ch) {
#pragma unroll
            for (int i = 0; i < S::LD; i++) {
                const int slot = tid + S::T * i, r = slot / (4 * NB), q = slot % (4 * NB);
                const long j = j0 + 16 * ch + r;
                const unsigned it = idn[i];
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                float yv = 0.0f;
                if (j < j1) {
                    if (q < nq) {
                        v = reinterpret_cast<const float4 *>(ibase + (size_t)it * P.pitch)[q];
                        if (4 * q + 3 >= k) {   // the pads of the last float4 are never trusted
                            if (4 * q + 1 >= k) v.y = 0.0f;
                            if (4 * q + 2 >= k) v.z = 0.0f;
                            v.w = 0.0f;
                        }
                    }
                    if (q == 0) yv = D.label[j] - (lin + ibias[it]);
                }
                gq[i] = v; gy[i] = yv;
                idn[i] = j + 16 < j1 ? D.item[j + 16] : 0u;
            }
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int i = 0; i < S::LD; i++) {
                const int slot = tid + S::T * i, r = slot / (4 * NB), q = slot % (4 * NB);
                *reinterpret_cast<float4 *>(&L.stage[buf][r * S::LP + 4 * q]) = gq[i];
                if (q == 0) L.y[buf][r] = gy[i];
            }
        };
        fi_f4 acc[S::NS];
#pragma unroll
        for (int i = 0; i < S::NS; i++) acc[i] = (fi_f4){0.0f, 0.0f, 0.0f, 0.0f};
        float bacc = 0.0f;
        fetch(0);
        stash(0);
        __syncthreads();
        for (long ch = 0; ch < nch; ch++) {
            const int buf = (int)(ch & 1);
            if (ch + 1 < nch) fetch(ch + 1);
            const float *st = L.stage[buf];
#pragma unroll
            for (int kk = 0; kk < 4; kk++) {
                const float *row = st + (4 * kk + lgrp) * S::LP + lcol;
#pragma unroll
                for (int i = 0; i < S::NS; i++)
                    if (wave + S::W * i < S::NT)   // (uniform over the wave)
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[16 * bi[i]], row[16 * bj[i]], acc[i], 0, 0, 0);
            }
            if (tid < S::N) {
#pragma unroll
                for (int r = 0; r < 16; r++) bacc = fmaf(L.y[buf][r], st[r * S::LP + tid], bacc);
            }
            if (ch + 1 < nch) stash(buf ^ 1);   // the other stage: every wave left it at the previous barrier
            __syncthreads();
        }

        // ---- the blocks to LDS: register r of a lane is (row 4 lgrp + r, column lcol) of its block
#pragma unroll
        for (int i = 0; i < S::NS; i++)
            if (wave + S::W * i < S::NT) *reinterpret_cast<fi_f4 *>(&L.tri[((wave + S::W * i) << 8) + (lcol << 4) + 4 * lgrp]) = acc[i];
        if (tid < S::N) L.b[tid] = bacc;
        __syncthreads();
        if (tid < k) L.tri[fi_at(tid, tid)] += D.reg;
        __syncthreads();

        // ---- L D L^T in place, b as one more row
        for (int j = 0; j < k; j++) {
            const int cj = fi_blk(0, j >> 4) + ((j & 15) << 4);   // column j inside block row 0; block row m: + fi_blk(m, 0)
            const float rd = 1.0f / L.tri[fi_at(j, j)];
            const float zb = L.b[j];
            float vi[NB];
#pragma unroll
            for (int m = 0; m < NB; m++) {
                const int i = li + 16 * m;
                vi[m] = (i > j && i < k) ? L.tri[fi_blk(m, 0) + cj + li] : 0.0f;
            }
#pragma unroll
            for (int n = 0; n < S::NC; n++) {
                const int c = g + S::G * n;
                if (c > j && c < k) {
                    const float lc = L.tri[fi_blk(c >> 4, 0) + cj + (c & 15)] * rd;   // L_cj
#pragma unroll
                    for (int m = 0; m < NB; m++) {
                        const int i = li + 16 * m;
                        if (i >= c && i < k) {
                            float *e = &L.tri[fi_at(i, c)];
                            *e = fmaf(-vi[m], lc, *e);
                        }
                    }
                    if (li == 0) L.b[c] = fmaf(-zb, lc, L.b[c]);
                }
            }
            __syncthreads();
        }

        // ---- backwards, wave 0: lane l holds the elements l + 64 e of z, then of x
        if (wave == 0) {
            float z[S::NE], x[S::NE];
#pragma unroll
            for (int e = 0; e < S::NE; e++) {
                z[e] = lane + 64 * e < k ? L.b[lane + 64 * e] : 0.0f;
                x[e] = 0.0f;
            }
            for (int i = k - 1; i >= 0; i--) {
                float zs = z[0];
#pragma unroll
                for (int e = 1; e < S::NE; e++)
                    if ((i >> 6) == e) zs = z[e];
                const float xi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(zs), i & 63)) / L.tri[fi_at(i, i)];
#pragma unroll
                for (int e = 0; e < S::NE; e++) {
                    const int c = lane + 64 * e;
                    if (c == i) x[e] = xi;
                    if (c < i) z[e] = fmaf(-L.tri[fi_at(i, c)], xi, z[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < S::NE; e++) {
                const int c = lane + 64 * e;
                if (c < k) {
                    out[c] = x[e];
                    if (D.write) wrow[c] = x[e];
                }
            }
        }
        __syncthreads();   // the next section reuses the stage, b and the triangle
    }
}

int fold_in_width_class(int k) { return k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 8; }

template <int NB>
static void fold_in_launch(const DevParams &P, const FoldInDev &D, hipStream_t st) {
    const unsigned grid = (unsigned)std::min<long>(D.nsec, 1L << 22);
    hipLaunchKernelGGL((k_fold_in<NB>), dim3(grid), dim3(FiShape<NB>::T), 0, st, P, D);
}

void launch_fold_in(const DevParams &P, const FoldInDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    switch (fold_in_width_class(P.k)) {
    case 1: fold_in_launch<1>(P, D, st); break;
    case 2: fold_in_launch<2>(P, D, st); break;
    case 4: fold_in_launch<4>(P, D, st); break;
    default: fold_in_launch<8>(P, D, st); break;
    }
}

}  // namespace svdf

// svdf_k_rankeval.hip -- batch ranking evaluation on the live model: the rank positions of held-out positives
// among ALL items, for many (user, positives, banned items) sections in one call.
//
// The score of candidate i for the user u of a section is proc_rank's (apex_svd_base.h:754-765) for a USER line u:1 and ITEM lines i:1:
// i_bias[i] + <W_user[u], W_item[i]> in the ranker's fp32 order -- four serial chains over the 4-float chunks, (a0 + a2) + (a1 + a3),
// the scalar tail in index order, bias + sum (rank_lane_score, svdf_k_rank.hip).  Every kernel below forms a score with exactly those
// operations in that order, so a candidate has ONE score whichever kernel computes it; no MFMA (its accumulation order is the
// hardware's).  The sweep counts, per positive, the candidates that score higher / equal / equal with a smaller id; banned candidates
// are counted like all others and taken back by k_rank_eval_ban.  Counters are integers; there is no floating-point atomic.
#include <algorithm>

#include "svdf_kernels.h"
#include "svdf_k_rankscore.h"

namespace svdf {

constexpr int RE_TS = 64;     // sections (rows) of a tile
constexpr int RE_SB = 4;      // sections a lane scores at once (register block)
constexpr int RE_PCH = RANK_EVAL_TILE_POS;   // thresholds (positives) a tile keeps in LDS

// re_row_score (one candidate against one user by ONE lane), re_section_row, re_item_row: svdf_k_rankscore.h

// the positives' own scores: the thresholds of the sweep.  One lane per (section, positive) pair.
__global__ __launch_bounds__(256) void k_rank_eval_pos(const DevParams P, const RankEvalDev D) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= D.npos) return;
    const int item = D.pos_item[q];
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    D.pos_score[q] = re_row_score(P.k, re_section_row(P, D.user_rows, D.sec_user, D.pos_sec[q]), re_item_row(ibase, P.pitch, item), ibias[item]);
}

// what lane `lane` adds for one score against the thresholds [q0, q1) of its section; cnt[] = greater | tied | tied with a smaller id
template <int IB, typename Add>
__device__ __forceinline__ void re_count(const float (&s)[IB], const bool (&on)[IB], const int (&cid)[IB], int q0, int q1, const float *ps, const int *pid,
                                         int lane, Add add) {
    for (int q = q0; q < q1; q++) {
        const float t = ps[q];
        const int p = pid[q];
        int ngt = 0, neq = 0, nbf = 0;
#pragma unroll
        for (int ib = 0; ib < IB; ib++) {
            const bool gt = on[ib] && s[ib] > t;
            const bool eq = on[ib] && s[ib] == t && cid[ib] != p;   // +0 == -0, NaN equals nothing
            ngt += __popcll(__ballot(gt));
            neq += __popcll(__ballot(eq));
            nbf += __popcll(__ballot(eq && cid[ib] < p));
        }
        if (lane == 0) add(q, ngt, neq, nbf);
    }
}

// The counting sweep for rows of up to 256 floats.  A workgroup (4 waves) owns a tile of up to 64 rows (sections, or slices of a section's
// positives) and the item range blockIdx.y; wave w scores rows 16 w .. 16 w + 15, four at a time, against 64 IB candidates (lane l owns
// candidates l, l + 64, ..).  The user rows, the thresholds and the counters stay in LDS for the whole item range; each tile of item rows is
// staged once, chunk-major ([chunk][candidate], one float4 of padding per chunk row so the staging stores spread over the banks), by loads
// that walk W_item's row-major block linearly.
template <int IB>
__global__ __launch_bounds__(256) void k_rank_eval_sweep(const DevParams P, const RankEvalDev D, long items_per_block) {
    constexpr int TI = 64 * IB;
    extern __shared__ float4 re_lds[];
    const int nch = P.pitch >> 2, nfull = P.k >> 2, ntail = P.k & 3;
    float4 *l_item = re_lds;                                   // [nch][TI + 1]
    float4 *l_user = l_item + (size_t)nch * (TI + 1);          // [RE_TS][nch]
    float *l_ps = reinterpret_cast<float *>(l_user + (size_t)RE_TS * nch);   // [RE_PCH]
    int *l_pid = reinterpret_cast<int *>(l_ps + RE_PCH);       // [RE_PCH]
    int *l_cnt = l_pid + RE_PCH;                               // [3][RE_PCH]
    int *l_nan = l_cnt + 3 * RE_PCH;                           // [RE_TS]
    int *l_first = l_nan + RE_TS;                              // [RE_TS]
    int *l_rp = l_first + RE_TS;                               // [RE_TS + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = D.tile_r0[blockIdx.x], nrows = D.tile_r0[blockIdx.x + 1] - r0;
    const int P0 = D.row_p0[r0], NP = D.row_p0[r0 + nrows] - P0;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);

    for (int q = tid; q < RE_TS * nch; q += 256) {
        const int sec = q / nch, ch = q - sec * nch;
        float4 v = zero4;
        if (sec < nrows) v = re_section_row(P, D.user_rows, D.sec_user, D.row_sec[r0 + sec])[ch];
        l_user[q] = v;
    }
    for (int q = tid; q < NP; q += 256) { l_ps[q] = D.pos_score[P0 + q]; l_pid[q] = D.pos_item[P0 + q]; }
    for (int q = tid; q < 3 * RE_PCH; q += 256) l_cnt[q] = 0;
    for (int q = tid; q < RE_TS; q += 256) { l_nan[q] = 0; l_first[q] = q < nrows ? D.row_first[r0 + q] : 0; }
    for (int q = tid; q <= RE_TS; q += 256) l_rp[q] = D.row_p0[r0 + (q < nrows ? q : nrows)] - P0;

    const long i_begin = (long)blockIdx.y * items_per_block;
    const long i_end = i_begin + items_per_block < (long)P.num_item ? i_begin + items_per_block : (long)P.num_item;
    for (long it0 = i_begin; it0 < i_end; it0 += TI) {
        __syncthreads();   // the previous tile has been read (first trip: nothing yet)
        const int live = i_end - it0 < TI ? (int)(i_end - it0) : TI;
        const float4 *src = re_item_row(ibase, P.pitch, it0);
        for (int q = tid; q < TI * nch; q += 256) {
            const int row = q / nch, ch = q - row * nch;
            float4 v = zero4;   // rows past the item range are zeros, never read from memory
            if (row < live) v = src[q];
            l_item[(size_t)ch * (TI + 1) + row] = v;
        }
        float bias[IB];
        bool on[IB];
        int cid[IB];
#pragma unroll
        for (int ib = 0; ib < IB; ib++) {
            const long c = it0 + lane + 64 * ib;
            on[ib] = c < i_end;
            cid[ib] = (int)c;
            bias[ib] = on[ib] ? ibias[c] : 0.0f;
        }
        __syncthreads();
        for (int g = 0; g < 16 / RE_SB; g++) {
            const int sec0 = wave * 16 + g * RE_SB;
            if (sec0 >= nrows) break;   // wave-uniform
            float acc[IB][RE_SB][4];
#pragma unroll
            for (int ib = 0; ib < IB; ib++)
#pragma unroll
                for (int sb = 0; sb < RE_SB; sb++) acc[ib][sb][0] = acc[ib][sb][1] = acc[ib][sb][2] = acc[ib][sb][3] = 0.0f;
            for (int j = 0; j < nfull; j++) {
                float4 v[IB];
#pragma unroll
                for (int ib = 0; ib < IB; ib++) v[ib] = l_item[(size_t)j * (TI + 1) + lane + 64 * ib];
#pragma unroll
                for (int sb = 0; sb < RE_SB; sb++) {
                    const float4 p = l_user[(sec0 + sb) * nch + j];
#pragma unroll
                    for (int ib = 0; ib < IB; ib++) {
                        acc[ib][sb][0] = acc[ib][sb][0] + p.x * v[ib].x;
                        acc[ib][sb][1] = acc[ib][sb][1] + p.y * v[ib].y;
                        acc[ib][sb][2] = acc[ib][sb][2] + p.z * v[ib].z;
                        acc[ib][sb][3] = acc[ib][sb][3] + p.w * v[ib].w;
                    }
                }
            }
            float4 vt[IB];
#pragma unroll
            for (int ib = 0; ib < IB; ib++) {
                vt[ib] = zero4;
                if (ntail) vt[ib] = l_item[(size_t)nfull * (TI + 1) + lane + 64 * ib];
            }
#pragma unroll
            for (int sb = 0; sb < RE_SB; sb++) {
                const int sec = sec0 + sb;
                if (sec < nrows) {   // wave-uniform
                    float s[IB];
                    float4 pt = zero4;
                    if (ntail) pt = l_user[sec * nch + nfull];
#pragma unroll
                    for (int ib = 0; ib < IB; ib++) {
                        float sum = (acc[ib][sb][0] + acc[ib][sb][2]) + (acc[ib][sb][1] + acc[ib][sb][3]);
                        if (ntail) {
                            sum = sum + pt.x * vt[ib].x;
                            if (ntail > 1) sum = sum + pt.y * vt[ib].y;
                            if (ntail > 2) sum = sum + pt.z * vt[ib].z;
                        }
                        s[ib] = 0.0f + (bias[ib] + sum);
                    }
                    // the row's counters belong to this wave alone: lane 0 adds without atomics
                    re_count<IB>(s, on, cid, l_rp[sec], l_rp[sec + 1], l_ps, l_pid, lane, [&](int q, int ngt, int neq, int nbf) {
                        if (ngt) l_cnt[q] += ngt;
                        if (neq) l_cnt[RE_PCH + q] += neq;
                        if (nbf) l_cnt[2 * RE_PCH + q] += nbf;
                    });
                    int nn = 0;
#pragma unroll
                    for (int ib = 0; ib < IB; ib++) nn += __popcll(__ballot(on[ib] && s[ib] != s[ib]));
                    if (lane == 0 && nn && l_first[sec]) l_nan[sec] += nn;
                }
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < NP; q += 256) {
        if (l_cnt[q]) atomicAdd(&D.greater[P0 + q], l_cnt[q]);
        if (l_cnt[RE_PCH + q]) atomicAdd(&D.tied[P0 + q], l_cnt[RE_PCH + q]);
        if (l_cnt[2 * RE_PCH + q]) atomicAdd(&D.before[P0 + q], l_cnt[2 * RE_PCH + q]);
    }
    for (int q = tid; q < nrows; q += 256)
        if (l_nan[q]) atomicAdd(&D.nan_cnt[D.row_sec[r0 + q]], l_nan[q]);
}

// The same count for wide rows (num_factor 257 .. 1024), which no LDS tile holds 64 of: one lane per (candidate, row), both factor rows
// read from HBM / L2 where they lie.  Right, not fast.
__global__ __launch_bounds__(256) void k_rank_eval_sweep_wide(const DevParams P, const RankEvalDev D) {
    const int r = blockIdx.y, lane = threadIdx.x & 63;
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int sec = D.row_sec[r];
    const bool on[1] = {c < (long)P.num_item};
    const int cid[1] = {(int)c};
    float s[1] = {0.0f};
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    if (on[0]) s[0] = re_row_score(P.k, re_section_row(P, D.user_rows, D.sec_user, sec), re_item_row(ibase, P.pitch, c), ibias[c]);
    re_count<1>(s, on, cid, D.row_p0[r], D.row_p0[r + 1], D.pos_score, D.pos_item, lane, [&](int q, int ngt, int neq, int nbf) {
        if (ngt) atomicAdd(&D.greater[q], ngt);
        if (neq) atomicAdd(&D.tied[q], neq);
        if (nbf) atomicAdd(&D.before[q], nbf);
    });
    const int nn = __popcll(__ballot(on[0] && s[0] != s[0]));
    if (lane == 0 && nn && D.row_first[r]) atomicAdd(&D.nan_cnt[sec], nn);
}

// Banned candidates are not ranked: each distinct (section, banned id) pair takes back what the sweep counted for it.  A positive is
// never banned (validated on the host), so `tied` needs no c != p test here.
__global__ __launch_bounds__(256) void k_rank_eval_ban(const DevParams P, const RankEvalDev D) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= D.nban) return;
    const int sec = D.ban_sec[b], c = D.ban_item[b];
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    const float s = re_row_score(P.k, re_section_row(P, D.user_rows, D.sec_user, sec), re_item_row(ibase, P.pitch, c), ibias[c]);
    if (s != s) { atomicSub(&D.nan_cnt[sec], 1); return; }
    for (int q = D.sec_p0[sec]; q < D.sec_p0[sec + 1]; q++) {
        const float t = D.pos_score[q];
        if (s > t) atomicSub(&D.greater[q], 1);
        else if (s == t) {
            atomicSub(&D.tied[q], 1);
            if (c < D.pos_item[q]) atomicSub(&D.before[q], 1);
        }
    }
}

static size_t re_lds_bytes(int pitch, int ib) {
    const size_t nch = (size_t)pitch >> 2;
    return 16 * (nch * (64 * (size_t)ib + 1) + (size_t)RE_TS * nch) + 4 * (5 * (size_t)RE_PCH + 3 * (size_t)RE_TS + 1);
}
int rank_eval_tile_rows(const DevParams &P) { return P.pitch <= 256 ? RE_TS : 1; }

static int re_ib(const DevParams &P) { return P.pitch <= 128 ? 2 : 1; }   // candidates per lane and step of the narrow sweep

// The item ranges of the narrow sweep over `ntile` tiles of rows: about 2048 workgroups in all, and at least 8 item tiles per workgroup
// where the items allow (the user rows are staged per workgroup).  The wide sweep has one range: every item lies in its grid.x.
void rank_eval_geometry(const DevParams &P, long ntile, int *gy, long *items_per_block) {
    if (P.pitch > 256) { *gy = 1; *items_per_block = P.num_item; return; }
    const long ti = 64 * re_ib(P), ntile_i = (P.num_item + ti - 1) / ti;
    long ysplit = std::max<long>(1, std::min<long>((2048 + ntile - 1) / std::max<long>(1, ntile), (ntile_i + 7) / 8));
    ysplit = std::min<long>(ysplit, 65535);
    const long per = ((ntile_i + ysplit - 1) / ysplit) * ti;
    *items_per_block = per;
    *gy = (int)((P.num_item + per - 1) / per);
}

void launch_rank_eval(const DevParams &P, const RankEvalDev &D, hipStream_t st) {
    if (D.npos <= 0) return;
    hipLaunchKernelGGL(k_rank_eval_pos, dim3((unsigned)((D.npos + 255) / 256)), dim3(256), 0, st, P, D);
    if (P.pitch <= 256) {
        const int ib = re_ib(P);
        int gy;
        long per;
        rank_eval_geometry(P, D.ntile, &gy, &per);
        const size_t lds = re_lds_bytes(P.pitch, ib);
        if (ib == 2) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rank_eval_sweep<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_rank_eval_sweep<2>, dim3((unsigned)D.ntile, (unsigned)gy), dim3(256), lds, st, P, D, per);
        } else {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rank_eval_sweep<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_rank_eval_sweep<1>, dim3((unsigned)D.ntile, (unsigned)gy), dim3(256), lds, st, P, D, per);
        }
    } else {
        for (int r = 0; r < D.nrow; r += RANK_EVAL_WIDE_ROWS) {   // grid.y is at most 65535
            RankEvalDev E = D;
            E.row_sec += r; E.row_p0 += r; E.row_first += r;
            hipLaunchKernelGGL(k_rank_eval_sweep_wide, dim3((unsigned)((P.num_item + 255) / 256), (unsigned)std::min(RANK_EVAL_WIDE_ROWS, D.nrow - r)), dim3(256), 0, st, P, E);
        }
    }
    if (D.nban > 0) hipLaunchKernelGGL(k_rank_eval_ban, dim3((unsigned)((D.nban + 255) / 256)), dim3(256), 0, st, P, D);
}

}  // namespace svdf

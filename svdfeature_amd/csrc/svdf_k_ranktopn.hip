// svdf_k_ranktopn.hip -- top-N item lists on the live model: for many (user, banned items) sections in one call, the
// top_n best items among ALL items that are not banned.
//
// The score of a candidate is section 6w's (svdf_k_rankscore.h, svdf_k_rankeval.hip): the narrow sweep below is k_rank_eval_sweep's tiling
// and scoring loop, operation for operation, so a candidate has ONE score whichever kernel computes it; no MFMA.  What differs is what
// happens to a score: it becomes a 64-bit KEY, (order-preserving word of the score) << 32 | ~id, so that a larger key is a better rank
// (higher score first, equal scores by ascending id, -0 folded onto +0) and the keys of a section are distinct.  The top N of a section are
// its N largest keys -- a pure function of the scores, whatever the grid.  A user x item score matrix never exists: per (section, item
// range) the owning wave keeps a THRESHOLD key in LDS and a short list of the keys that beat it in an HBM workspace; a full list is cut to
// its N largest by a bitonic sort in a wave-private LDS buffer, which raises the threshold.  The merge kernel selects over a section's lists.
// Banned candidates are excluded in the sweep.  Integer atomics only (the NaN count).
#include <algorithm>

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

constexpr int TN_TS = 64;                    // sections of a tile
constexpr int TN_SB = 4;                     // sections a lane scores at once (register block)
// tn_key_t, tn_key, tn_key_score, tn_key_id, tn_wave_sync, tn_sort_keep and TN_SORT: svdf_k_rankkey.h

// What the wave that owns a list does with one step's scores (IB candidates per lane): the keys of ranked candidates that beat the
// threshold are appended through a ballot prefix; a list without room for a whole step is first cut to its top_n largest.  `list` is the
// (section, item range)'s slice of the workspace, *cnt_p and *thr_p its state in LDS, `scratch` the wave's sort buffer.  cap >= top_n + 64 IB.
template <int IB>
__device__ __forceinline__ void tn_select(const float (&s)[IB], const bool (&on)[IB], const int (&cid)[IB], tn_key_t *list, int *cnt_p, tn_key_t *thr_p,
                                          tn_key_t *scratch, int top_n, int cap, int lane) {
    int cnt = __builtin_amdgcn_readfirstlane(*cnt_p);
    tn_key_t thr = *thr_p;
    if (cnt + 64 * IB > cap) {   // wave-uniform
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // the wave's own appends, by other lanes, are read back below
        for (int i = lane; i < cnt; i += 64) scratch[i] = list[i];
        cnt = tn_sort_keep(scratch, cnt, top_n, lane, thr);
        for (int i = lane; i < cnt; i += 64) list[i] = scratch[i];
        if (lane == 0) *thr_p = thr;
        tn_wave_sync();
    }
    const tn_key_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int ib = 0; ib < IB; ib++) {
        const tn_key_t key = tn_key(s[ib], cid[ib]);
        const bool take = on[ib] && s[ib] == s[ib] && key > thr;   // a NaN is never listed (it flags the section)
        const tn_key_t b = __ballot(take);
        if (take) list[cnt + __popcll(b & below)] = key;           // cnt + popc(b) <= cap
        cnt += __popcll(b);
    }
    if (lane == 0) *cnt_p = cnt;
    tn_wave_sync();
}

// first entry >= x of the ascending ids ban[b0 .. b1)
__device__ __forceinline__ int tn_lower_bound(const int *__restrict__ ban, int b0, int b1, long x) {
    while (b0 < b1) {
        const int m = b0 + ((b1 - b0) >> 1);
        if ((long)ban[m] < x) b0 = m + 1; else b1 = m;
    }
    return b0;
}

// The selecting sweep for rows of up to 256 floats: k_rank_eval_sweep's tiling.  A workgroup (4 waves) owns the sections 64 blockIdx.x ..
// + 63 and the item range blockIdx.y; wave w scores sections 16 w .. 16 w + 15, four at a time, against 64 IB candidates (lane l owns
// candidates l, l + 64, ..).  User rows stay in LDS; each tile of item rows is staged once, chunk-major.  Thread t < 64 walks the sorted ban
// list of section t with a cursor in a register and sets, per item tile, the section's bits of a [64][64 IB] mask; the scoring loop is
// mask-free.  The list state of a section (count, threshold) belongs to the wave that owns the section.
template <int IB>
__global__ __launch_bounds__(256) void k_rank_topn_sweep(const DevParams P, const RankTopnDev D) {
    constexpr int TI = 64 * IB;
    extern __shared__ float4 tn_lds[];
    const int nch = P.pitch >> 2, nfull = P.k >> 2, ntail = P.k & 3;
    float4 *l_item = tn_lds;                                   // [nch][TI + 1]
    float4 *l_user = l_item + (size_t)nch * (TI + 1);          // [TN_TS][nch]
    tn_key_t *l_scr = reinterpret_cast<tn_key_t *>(l_user + (size_t)TN_TS * nch);   // [4][TN_SORT]
    tn_key_t *l_thr = l_scr + 4 * TN_SORT;                     // [TN_TS]
    tn_key_t *l_mask = l_thr + TN_TS;                          // [TN_TS][IB]
    int *l_cnt = reinterpret_cast<int *>(l_mask + TN_TS * IB); // [TN_TS]
    int *l_nan = l_cnt + TN_TS;                                // [TN_TS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sec_base = blockIdx.x * TN_TS;
    const int nrows = D.nsec - sec_base < TN_TS ? D.nsec - sec_base : TN_TS;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);

    for (int q = tid; q < TN_TS * nch; q += 256) {
        const int sec = q / nch, ch = q - sec * nch;
        float4 v = zero4;
        if (sec < nrows) v = re_section_row(P, D.user_rows, D.sec_user, sec_base + sec)[ch];
        l_user[q] = v;
    }
    for (int q = tid; q < TN_TS; q += 256) { l_thr[q] = 0ull; l_cnt[q] = 0; l_nan[q] = 0; }

    const long i_begin = (long)blockIdx.y * D.items_per_block;
    const long i_end = i_begin + D.items_per_block < (long)P.num_item ? i_begin + D.items_per_block : (long)P.num_item;
    int bcur = 0, bend = 0;   // thread t < nrows: what is left of section t's ban list
    if (tid < nrows) {
        bend = D.ban_p0[sec_base + tid + 1];
        bcur = tn_lower_bound(D.ban_item, D.ban_p0[sec_base + tid], bend, i_begin);
    }
    for (long it0 = i_begin; it0 < i_end; it0 += TI) {
        __syncthreads();   // the previous tile and its mask have been read (first trip: nothing yet)
        const int live = i_end - it0 < TI ? (int)(i_end - it0) : TI;
        const float4 *src = re_item_row(ibase, P.pitch, it0);
        for (int q = tid; q < TI * nch; q += 256) {
            const int row = q / nch, ch = q - row * nch;
            float4 v = zero4;   // rows past the item range are zeros, never read from memory
            if (row < live) v = src[q];
            l_item[(size_t)ch * (TI + 1) + row] = v;
        }
        if (tid < TN_TS) {
            tn_key_t m[IB];
#pragma unroll
            for (int ib = 0; ib < IB; ib++) m[ib] = 0ull;
            while (bcur < bend) {
                const long d = (long)D.ban_item[bcur] - it0;   // >= 0: the cursor has passed everything below it0
                if (d >= TI) break;
#pragma unroll
                for (int ib = 0; ib < IB; ib++)
                    if ((int)(d >> 6) == ib) m[ib] |= 1ull << (d & 63);
                bcur++;
            }
#pragma unroll
            for (int ib = 0; ib < IB; ib++) l_mask[tid * IB + ib] = m[ib];
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
        for (int g = 0; g < 16 / TN_SB; g++) {
            const int sec0 = wave * 16 + g * TN_SB;
            if (sec0 >= nrows) break;   // wave-uniform
            float acc[IB][TN_SB][4];
#pragma unroll
            for (int ib = 0; ib < IB; ib++)
#pragma unroll
                for (int sb = 0; sb < TN_SB; sb++) acc[ib][sb][0] = acc[ib][sb][1] = acc[ib][sb][2] = acc[ib][sb][3] = 0.0f;
            for (int j = 0; j < nfull; j++) {
                float4 v[IB];
#pragma unroll
                for (int ib = 0; ib < IB; ib++) v[ib] = l_item[(size_t)j * (TI + 1) + lane + 64 * ib];
#pragma unroll
                for (int sb = 0; sb < TN_SB; sb++) {
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
            for (int sb = 0; sb < TN_SB; sb++) {
                const int sec = sec0 + sb;
                if (sec < nrows) {   // wave-uniform
                    float s[IB];
                    bool ranked[IB];
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
                        ranked[ib] = on[ib] && !((l_mask[sec * IB + ib] >> lane) & 1ull);
                    }
                    int nn = 0;
#pragma unroll
                    for (int ib = 0; ib < IB; ib++) nn += __popcll(__ballot(ranked[ib] && s[ib] != s[ib]));
                    if (lane == 0 && nn) l_nan[sec] += nn;   // the section's state belongs to this wave alone
                    tn_select<IB>(s, ranked, cid, D.list + ((size_t)(sec_base + sec) * D.gy + blockIdx.y) * D.cap, &l_cnt[sec], &l_thr[sec],
                                  l_scr + wave * TN_SORT, D.top_n, D.cap, lane);
                }
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < nrows; q += 256) {
        D.list_cnt[(size_t)(sec_base + q) * D.gy + blockIdx.y] = l_cnt[q];
        if (l_nan[q]) atomicAdd(&D.nan_cnt[sec_base + q], l_nan[q]);
    }
}

// The same selection for wide rows (num_factor 257 .. 1024), which no LDS tile holds 64 of: one wave per (section, item range) walks its
// range 64 candidates at a time, both factor rows read from HBM / L2 where they lie; a ban is looked up in the section's sorted list.
// Right, not fast.
__global__ __launch_bounds__(64) void k_rank_topn_sweep_wide(const DevParams P, const RankTopnDev D) {
    __shared__ tn_key_t l_scr[TN_SORT];
    __shared__ tn_key_t l_thr;
    __shared__ int l_cnt;
    const int sec = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) { l_thr = 0ull; l_cnt = 0; }
    __syncthreads();
    const long i_begin = (long)blockIdx.y * D.items_per_block;
    const long i_end = i_begin + D.items_per_block < (long)P.num_item ? i_begin + D.items_per_block : (long)P.num_item;
    const int b0 = D.ban_p0[sec], b1 = D.ban_p0[sec + 1];
    const float4 *urow = re_section_row(P, D.user_rows, D.sec_user, sec);
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    tn_key_t *list = D.list + ((size_t)sec * D.gy + blockIdx.y) * D.cap;
    int nn = 0;
    for (long c0 = i_begin; c0 < i_end; c0 += 64) {
        const long c = c0 + lane;
        bool ranked[1] = {c < i_end};
        if (ranked[0]) {
            const int at = tn_lower_bound(D.ban_item, b0, b1, c);
            ranked[0] = !(at < b1 && (long)D.ban_item[at] == c);
        }
        const int cid[1] = {(int)c};
        float s[1] = {0.0f};
        if (ranked[0]) s[0] = re_row_score(P.k, urow, re_item_row(ibase, P.pitch, c), ibias[c]);
        nn += __popcll(__ballot(ranked[0] && s[0] != s[0]));
        tn_select<1>(s, ranked, cid, list, &l_cnt, &l_thr, l_scr, D.top_n, D.cap, lane);
    }
    if (lane == 0) {
        D.list_cnt[(size_t)sec * D.gy + blockIdx.y] = l_cnt;
        if (nn) atomicAdd(&D.nan_cnt[sec], nn);
    }
}

// One wave per section: the top_n largest keys over the section's gy lists, in rank order.  The keys stream through the wave's LDS buffer
// the way candidates stream through a list in the sweep: those above the threshold are appended, a full buffer is sorted and cut.
__global__ __launch_bounds__(64) void k_rank_topn_merge(const RankTopnDev D) {
    __shared__ tn_key_t buf[TN_SORT];
    const int sec = blockIdx.x, lane = threadIdx.x, N = D.top_n;
    const tn_key_t below = (1ull << lane) - 1ull;
    int cnt = 0;
    tn_key_t thr = 0ull;
    const bool bad = D.nan_cnt[sec] != 0;   // a ranked candidate scored NaN: the section lists nothing
    if (!bad)
        for (int y = 0; y < D.gy; y++) {
            const int n = D.list_cnt[(size_t)sec * D.gy + y];
            const tn_key_t *list = D.list + ((size_t)sec * D.gy + y) * D.cap;
            for (int i0 = 0; i0 < n; i0 += 64) {
                if (cnt + 64 > TN_SORT) cnt = tn_sort_keep(buf, cnt, N, lane, thr);
                const tn_key_t key = i0 + lane < n ? list[i0 + lane] : 0ull;
                const bool take = key > thr;
                const tn_key_t b = __ballot(take);
                if (take) buf[cnt + __popcll(b & below)] = key;
                cnt += __popcll(b);
                tn_wave_sync();
            }
        }
    cnt = tn_sort_keep(buf, cnt, N, lane, thr);
    for (int r = lane; r < N; r += 64) {
        const tn_key_t key = r < cnt ? buf[r] : 0ull;
        D.item_out[(size_t)sec * N + r] = r < cnt ? tn_key_id(key) : -1;
        D.score_out[(size_t)sec * N + r] = r < cnt ? tn_key_score(key) : 0.0f;
    }
    if (lane == 0) D.count_out[sec] = cnt;
}

static size_t tn_lds_bytes(int pitch, int ib) {
    const size_t nch = (size_t)pitch >> 2;
    return 16 * (nch * (64 * (size_t)ib + 1) + (size_t)TN_TS * nch) + 8 * (4 * (size_t)TN_SORT + (size_t)TN_TS + (size_t)TN_TS * ib) + 4 * 2 * (size_t)TN_TS;
}
static int tn_ib(const DevParams &P) { return P.pitch <= 128 ? 2 : 1; }   // candidates per lane and step; the wide sweep takes 1
int rank_topn_tile_rows(const DevParams &P) { return P.pitch <= 256 ? TN_TS : 1; }   // sections of one workgroup (narrow) or wave (wide)

// room for top_n kept keys and one step's appends, and for as many appends again between two cuts where TN_SORT allows
int rank_topn_cap(const DevParams &P, int top_n) {
    const int ti = P.pitch <= 256 ? 64 * tn_ib(P) : 64;
    int cap = 128;
    while (cap < 2 * top_n + ti) cap <<= 1;
    return std::min(std::max(cap, top_n + ti), TN_SORT);
}

void rank_topn_geometry(const DevParams &P, long nsec, long max_lists, int *gy, long *items_per_block) {
    const long ti = P.pitch <= 256 ? 64 * tn_ib(P) : 64, ntile_i = (P.num_item + ti - 1) / ti;
    // narrow: about 2048 workgroups in all, at least 8 item tiles per workgroup where the items allow (the user rows are staged per
    // workgroup); wide: about 8192 waves
    const long ts = rank_topn_tile_rows(P), units = (nsec + ts - 1) / ts, want = P.pitch <= 256 ? 2048 : 8192;
    long ysplit = std::max<long>(1, std::min<long>((want + units - 1) / units, (ntile_i + 7) / 8));
    ysplit = std::min<long>(ysplit, std::max<long>(1, max_lists / std::max<long>(1, nsec)));
    ysplit = std::min<long>(ysplit, 65535);
    const long per = ((ntile_i + ysplit - 1) / ysplit) * ti;
    *items_per_block = per;
    *gy = (int)((P.num_item + per - 1) / per);
}

void launch_rank_topn(const DevParams &P, const RankTopnDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    if (P.pitch <= 256) {
        const int ib = tn_ib(P);
        const size_t lds = tn_lds_bytes(P.pitch, ib);
        const dim3 grid((unsigned)((D.nsec + rank_topn_tile_rows(P) - 1) / rank_topn_tile_rows(P)), (unsigned)D.gy);
        if (ib == 2) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rank_topn_sweep<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_rank_topn_sweep<2>, grid, dim3(256), lds, st, P, D);
        } else {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rank_topn_sweep<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_rank_topn_sweep<1>, grid, dim3(256), lds, st, P, D);
        }
    } else {
        hipLaunchKernelGGL(k_rank_topn_sweep_wide, dim3((unsigned)D.nsec, (unsigned)D.gy), dim3(64), 0, st, P, D);
    }
    hipLaunchKernelGGL(k_rank_topn_merge, dim3((unsigned)D.nsec), dim3(64), 0, st, D);
}

}  // namespace svdf

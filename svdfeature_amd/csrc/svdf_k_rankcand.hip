// svdf_k_rankcand.hip -- ranking over per-section candidate lists on the live model: for many sections in one call,
// the rank positions of held-out positives among the section's OWN candidates, or the top_n best of them.  Only the listed (section,
// candidate) pairs are scored: the hot path is a gather of item rows, not a sweep of the catalogue.
//
// The score of a pair is section 6w's (svdf_k_rankscore.h): four serial chains over the 4-float chunks, (a0 + a2) + (a1 + a3), the scalar
// tail, 0 + (bias + sum), unfused -- by re_row_score in the one-lane form, by k_rank_eval_sweep's scoring loop over rows staged in LDS in
// the staged form -- so a pair has ONE score whichever kernel computes it; no MFMA.  The scores of a piece go to HBM once (cand_score); the
// count and the selection read them back, a wave per section.  A section belongs to one wave: no atomics at all.
#include <algorithm>

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

constexpr int RC_NB = 8;   // 16-byte requests a lane of the staged form has in flight: 8 KiB per wave

// The correctness baseline, and the form for wide rows (num_factor 257 .. 1024): one lane per pair, both factor rows read from HBM / L2
// where they lie.  Lane l of the wave that owns tile t scores the tile's pair l.
__global__ __launch_bounds__(256) void k_rank_cand_score_lane(const DevParams P, const RankCandDev D) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long t = g >> 6;
    if (t >= (long)D.ntile) return;
    const int q = D.tile_q0[t] + (int)(g & 63);
    if (q >= D.tile_q0[t + 1]) return;   // a pair past the tile's end is neither loaded nor scored
    const int item = D.cand_id[q];
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    D.cand_score[q] = re_row_score(P.k, re_section_row(P, D.user_rows, D.sec_user, D.tile_sec[t]), re_item_row(ibase, P.pitch, item), ibias[item]);
}

// The staged form for rows of up to 256 floats: ONE wave (a workgroup of its own) owns a tile of up to 64 pairs of one section.  The item
// rows are gathered by 16-byte loads -- consecutive lanes cover one row, pitch / 4 lanes per row, so each request is a whole contiguous row
// -- and staged chunk-major in the wave's LDS ([chunk][row], one float4 of padding per chunk row as in the sweeps), SUB rows in a turn;
// lane l then scores the tile's pair l from LDS against the section's row, whose address is the same for the whole wave.  SUB is sized so
// that the LDS image stays below 17.5 KiB at every width (64 rows up to pitch 64, 32 up to 128, 16 up to 256): 9 waves per CU by LDS.
template <int SUB>
__global__ __launch_bounds__(64) void k_rank_cand_score(const DevParams P, const RankCandDev D) {
    extern __shared__ float4 rc_item[];   // [nch][SUB + 1]
    const int lane = threadIdx.x;
    const int nch = P.pitch >> 2, nfull = P.k >> 2, ntail = P.k & 3;
    const int t = blockIdx.x;
    const int q0 = D.tile_q0[t], n = D.tile_q0[t + 1] - q0;   // 1 .. 64 pairs
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float *ibase = re_item_base(P, D.item_rows), *ibias = re_item_bias(P, D.item_bias);
    const float4 *urow = re_section_row(P, D.user_rows, D.sec_user, D.tile_sec[t]);
    const bool on = lane < n;
    const int cid = on ? D.cand_id[q0 + lane] : 0;
    const float bias = on ? ibias[cid] : 0.0f;
    for (int r0 = 0; r0 < n; r0 += SUB) {
        const int rows = n - r0 < SUB ? n - r0 : SUB, live = rows * nch;
        tn_wave_sync();   // the previous turn has been read (first trip: nothing yet)
        for (int e0 = 0; e0 < live; e0 += 64 * RC_NB) {   // every lane takes every trip: the shuffle reads lanes that stage nothing
            float4 v[RC_NB];
            int dst[RC_NB];
#pragma unroll
            for (int b = 0; b < RC_NB; b++) {             // RC_NB requests ahead of their LDS stores
                const int e = e0 + 64 * b + lane;
                const bool in = e < live;                 // a row past the tile's end is not loaded
                const int row = in ? e / nch : 0, ch = e - row * nch;
                const int item = __shfl(cid, r0 + row);
                v[b] = zero4;
                if (in) v[b] = re_item_row(ibase, P.pitch, item)[ch];
                dst[b] = in ? ch * (SUB + 1) + row : -1;
            }
#pragma unroll
            for (int b = 0; b < RC_NB; b++)
                if (dst[b] >= 0) rc_item[dst[b]] = v[b];
        }
        tn_wave_sync();
        if (lane >= r0 && lane < r0 + rows) {     // ... nor scored
            const int row = lane - r0;
            float acc[4];
            acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
            for (int j = 0; j < nfull; j++) {
                const float4 v = rc_item[(size_t)j * (SUB + 1) + row];
                const float4 p = urow[j];
                acc[0] = acc[0] + p.x * v.x;
                acc[1] = acc[1] + p.y * v.y;
                acc[2] = acc[2] + p.z * v.z;
                acc[3] = acc[3] + p.w * v.w;
            }
            float4 vt = zero4, pt = zero4;
            if (ntail) { vt = rc_item[(size_t)nfull * (SUB + 1) + row]; pt = urow[nfull]; }
            float sum = (acc[0] + acc[2]) + (acc[1] + acc[3]);
            if (ntail) {
                sum = sum + pt.x * vt.x;
                if (ntail > 1) sum = sum + pt.y * vt.y;
                if (ntail > 2) sum = sum + pt.z * vt.z;
            }
            D.cand_score[q0 + lane] = 0.0f + (bias + sum);
        }
    }
}

// Positions: a wave per section loops over the section's positives.  The threshold is the positive's own entry of cand_score (its index
// comes from the host: a positive's score is read, not recomputed); the lanes stride over the section's scores and ids and count greater /
// tied (c != p) / tied with a smaller id in integers, reduced in the wave.  +0 == -0, NaN equals nothing.  The same wave flags the section.
__global__ __launch_bounds__(64) void k_rank_cand_count(const RankCandDev D) {
    const int sec = blockIdx.x, lane = threadIdx.x;
    const int p0 = D.sec_p0[sec], p1 = D.sec_p0[sec + 1];
    const int q0 = D.sec_q0[sec], q1 = D.sec_q0[sec + 1];
    int nn = 0;
    for (int q = q0 + lane; q < q1; q += 64) {
        const float s = D.cand_score[q];
        nn |= s != s ? 1 : 0;
    }
    const bool bad = __ballot(nn) != 0ull;
    if (lane == 0) D.nan_out[sec] = bad ? 1 : 0;
    if (bad) {   // wave-uniform: a ranked candidate scored NaN, the section has no positions
        for (int p = p0 + lane; p < p1; p += 64) { D.position_out[p] = -1; D.tied_out[p] = -1; }
        return;
    }
    for (int p = p0; p < p1; p++) {
        const int at = D.pos_at[p];
        const float t = D.cand_score[at];
        const int pid = D.cand_id[at];
        int ngt = 0, neq = 0, nbf = 0;
        for (int q = q0 + lane; q < q1; q += 64) {
            const float s = D.cand_score[q];
            const int c = D.cand_id[q];
            const bool eq = s == t && c != pid;
            ngt += s > t ? 1 : 0;
            neq += eq ? 1 : 0;
            nbf += eq && c < pid ? 1 : 0;
        }
        for (int o = 32; o > 0; o >>= 1) {
            ngt += __shfl_xor(ngt, o);
            neq += __shfl_xor(neq, o);
            nbf += __shfl_xor(nbf, o);
        }
        if (lane == 0) { D.position_out[p] = ngt + nbf; D.tied_out[p] = neq; }
    }
}

// Top-N: a wave per section streams tn_key(score, id) over its pairs through the wave's LDS sort buffer, the way k_rank_topn_merge streams
// list keys: those above the threshold are appended, a full buffer is sorted and cut to top_n.  Ids and scores leave in rank order.
__global__ __launch_bounds__(64) void k_rank_cand_select(const RankCandDev D) {
    __shared__ tn_key_t buf[TN_SORT];
    const int sec = blockIdx.x, lane = threadIdx.x, N = D.top_n;
    const int q0 = D.sec_q0[sec], q1 = D.sec_q0[sec + 1];
    const tn_key_t below = (1ull << lane) - 1ull;
    int cnt = 0, nn = 0;
    tn_key_t thr = 0ull;
    for (int i0 = q0; i0 < q1; i0 += 64) {
        if (cnt + 64 > TN_SORT) cnt = tn_sort_keep(buf, cnt, N, lane, thr);
        const bool in = i0 + lane < q1;
        const float s = in ? D.cand_score[i0 + lane] : 0.0f;
        const tn_key_t key = in ? tn_key(s, D.cand_id[i0 + lane]) : 0ull;
        nn |= s != s ? 1 : 0;
        const bool take = in && s == s && key > thr;   // a NaN is never listed (it flags the section)
        const tn_key_t b = __ballot(take);
        if (take) buf[cnt + __popcll(b & below)] = key;
        cnt += __popcll(b);
        tn_wave_sync();
    }
    const bool bad = __ballot(nn) != 0ull;   // a ranked candidate scored NaN: the section lists nothing
    if (bad) cnt = 0;
    cnt = tn_sort_keep(buf, cnt, N, lane, thr);
    for (int r = lane; r < N; r += 64) {
        const tn_key_t key = r < cnt ? buf[r] : 0ull;
        D.item_out[(size_t)sec * N + r] = r < cnt ? tn_key_id(key) : -1;
        D.score_out[(size_t)sec * N + r] = r < cnt ? tn_key_score(key) : 0.0f;
    }
    if (lane == 0) { D.count_out[sec] = cnt; D.nan_out[sec] = bad ? 1 : 0; }
}

static int rc_sub(int pitch) { return pitch <= 64 ? 64 : pitch <= 128 ? 32 : 16; }

int rank_cand_form(const DevParams &P, int form) {
    if (P.pitch > 256) return 1;   // no LDS tile holds the rows
    if (form == 1 || form == 2) return form;
    return 2;
}

void launch_rank_cand(const DevParams &P, const RankCandDev &D, int form, hipStream_t st) {
    if (D.nsec <= 0) return;
    if (D.ntile > 0) {
        if (rank_cand_form(P, form) == 2) {
            const int sub = rc_sub(P.pitch);
            const size_t lds = 16 * ((size_t)P.pitch >> 2) * ((size_t)sub + 1);
            const dim3 grid((unsigned)D.ntile);
            if (sub == 64) hipLaunchKernelGGL(k_rank_cand_score<64>, grid, dim3(64), lds, st, P, D);
            else if (sub == 32) hipLaunchKernelGGL(k_rank_cand_score<32>, grid, dim3(64), lds, st, P, D);
            else hipLaunchKernelGGL(k_rank_cand_score<16>, grid, dim3(64), lds, st, P, D);
        } else {
            hipLaunchKernelGGL(k_rank_cand_score_lane, dim3((unsigned)(((long)D.ntile + 3) / 4)), dim3(256), 0, st, P, D);
        }
    }
    if (D.top_n > 0) hipLaunchKernelGGL(k_rank_cand_select, dim3((unsigned)D.nsec), dim3(64), 0, st, D);
    else hipLaunchKernelGGL(k_rank_cand_count, dim3((unsigned)D.nsec), dim3(64), 0, st, D);
}

}  // namespace svdf

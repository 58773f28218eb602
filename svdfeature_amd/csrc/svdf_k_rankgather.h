// svdf_k_rankgather.h -- the pinned scores of 64 listed candidates by ONE wave, shared by k_rank_topn_exact (svdf_k_ranktopn_exact.hip,
// DESIGN.md section 6ai) and k_rank_eval_band (svdf_k_rankeval_mfma.hip, section 6aj).  K goes in chunks of 64 floats: the wave gathers the
// chunk of its 64 rows coalesced -- 16 lanes a row, four rows a load, all 16 loads of a lane in flight -- into LDS at a pitch of 17 float4s
// (16 consecutive lanes then touch every bank once, writing and reading), and lane l carries candidate l's four chains across the chunks
// (re_row_chains / re_row_finish, the operations of re_row_score).  u is read from LDS as a broadcast.
#ifndef SVDF_K_RANKGATHER_H_
#define SVDF_K_RANKGATHER_H_

#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"

namespace svdf {

constexpr int TX_QC = 16;              // float4s of a K chunk (64 floats)
constexpr int TX_LP = TX_QC + 1;       // float4s between two candidate rows of the stage
constexpr int TX_LD = 64 * TX_QC / 64; // float4 loads of a lane per (64 candidates, chunk): 16, rows 4 t + lane / 16

// Candidates r0 .. r0 + 63 of a list of cnt, id_of(i) the item id of candidate i: returns the pinned score of candidate r0 + lane (`on`:
// there is one; `id`: its item).  l_u holds the user row ([pitch / 4] float4s), l_rows is the wave's stage of 64 * TX_LP float4s.
template <typename IdOf>
__device__ __forceinline__ float tx_pinned_scores(const DevParams &P, const float *ibase, const float *ibias, const float4 *l_u, float4 *l_rows, int r0,
                                                  int cnt, int lane, IdOf id_of, bool &on, int &id) {
    const int k = P.k, nq = P.pitch >> 2, nfull = k >> 2, ntail = k & 3;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int grp = lane >> 4, gq = lane & 15;
    const int nchunk = (nq + TX_QC - 1) / TX_QC;
    const int ci = r0 + lane;
    on = ci < cnt;
    id = on ? id_of(ci) : 0;
    const float bias = on ? ibias[id] : 0.0f;
    const float4 *src[TX_LD];   // the rows this lane loads from: candidate r0 + 4 t + grp
#pragma unroll
    for (int t = 0; t < TX_LD; t++) {
        const int row = r0 + 4 * t + grp;
        src[t] = row < cnt ? re_item_row(ibase, P.pitch, id_of(row)) : nullptr;
    }
    float4 a = zero4, pt = zero4, vt = zero4;
    for (int c = 0; c < nchunk; c++) {
        const int qb = c * TX_QC;
        float4 g[TX_LD];
#pragma unroll
        for (int t = 0; t < TX_LD; t++) {
            g[t] = zero4;
            if (src[t] && qb + gq < nq) g[t] = src[t][qb + gq];
        }
        tn_wave_sync();   // the previous chunk has been read
#pragma unroll
        for (int t = 0; t < TX_LD; t++) l_rows[(4 * t + grp) * TX_LP + gq] = g[t];
        tn_wave_sync();
        const int left = nfull - qb, n = left < 0 ? 0 : (left < TX_QC ? left : TX_QC);
        re_row_chains(a, l_u + qb, l_rows + lane * TX_LP, n);
        if (ntail && left >= 0 && left < TX_QC) { pt = l_u[nfull]; vt = l_rows[lane * TX_LP + left]; }
    }
    return re_row_finish(a, ntail, pt, vt, bias);
}

}  // namespace svdf
#endif

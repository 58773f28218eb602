// svdf_k_pairhard.hip -- the hard pass of a pair source: ONE kernel draws, scores and selects.  Pair q = r * num_neg + j
// of source row r has num_cand = C candidates, candidate i the plain rule's negative of pair index e = q * C + i (pair_src_pick, as
// k_pair_draw runs it with q); each is scored against user_r with the live model in the ranker's pinned order (svdf_k_rankscore.h), and the
// pair's negative is the candidate with the largest tn_key(score, id) among those that do not score NaN -- cand(q, 0) when all do.  Candidate
// ids and scores never go to HBM: only (user, pos, neg) at q and, on request, the chosen score.
//
// A WAVE OWNS WHOLE PAIRS.  A unit is max(1, 64 / C) consecutive pairs, lane l of its turn the entry (pair l / C, candidate l % C); a pair
// with C > 64 is a unit of its own and takes ceil(C / 64) turns with a running best key in its first lane.  The keys of a pair's lanes are
// reduced to their maximum by a segmented shuffle-down inside the wave -- equal keys are one id and hence one score, so the result is an id
// and does not depend on which of two equal candidates came first.  No pair is split over waves: no atomics, nothing depends on timing.
// Waves stride over the units; a workgroup is one wave.
//
// Two forms of the score, the same bits (four serial chains over the 4-float chunks, (a0 + a2) + (a1 + a3), the scalar tail, 0 + (bias +
// sum), unfused; no MFMA):
//   lane   (SUB = 0)  every lane calls re_row_score on the two rows where they lie; the baseline, and the form for rows above 256 floats
//   staged (SUB > 0)  the turn's item rows are gathered by 16-byte loads, consecutive lanes covering one row, into the wave's LDS in
//                     k_rank_cand_score's layout ([chunk][row], one float4 of padding, SUB rows a turn within the same 17.5 KiB); lane l
//                     scores entry l from LDS with the sweeps' loop.  The user row differs per pair, not per wave as in section 6aa: it is
//                     read through L1 / L2, the C lanes of a pair reading one address.
// The loop bound of a draw is the compile-time constant PAIR_SRC_DRAWS; an exhausted entry reports e + 1 through the one-word flag (plain
// store, any writer may win) and goes on with id 0, a valid row.
// A source with ITEM WEIGHTS (section 6ae) draws every candidate through its weight table (pair_weight_pick, svdf_pairweight_lists.h): the
// template argument WF is 0 without weights -- the kernel as it was --, 1 for the search of the whole cdf, 2 for the guided search.
#include <algorithm>

#include "svdf_kernels.h"
#include "svdf_k_rankkey.h"
#include "svdf_k_rankscore.h"
#include "svdf_pairweight_lists.h"

namespace svdf {

constexpr int PH_NB = 8;            // 16-byte requests a lane of the staged form has in flight: 8 KiB per wave
constexpr int PH_MAX_GRID = 8192;   // waves of a launch: 32 a CU; the rest of the units is strided over

template <int SUB, int WF>
__global__ __launch_bounds__(64) void k_pair_hard(const DevParams P, const PairHardDev H, const long nunit, const PairWeightDev T) {
    extern __shared__ float4 ph_item[];   // staged: [nch][SUB + 1]
    const PairDrawDev &D = H.D;
    const int lane = threadIdx.x;
    const int C = H.num_cand;
    const int ppt = C < 64 ? 64 / C : 1;   // whole pairs of a unit
    const int cnt0 = C < 64 ? C : 64;      // entries of a pair in its first turn
    const float *ibase = re_item_base(P, nullptr), *ibias = re_item_bias(P, nullptr);
    for (long unit = blockIdx.x; unit < nunit; unit += gridDim.x) {
        const long q0 = unit * ppt;
        const int np = D.npair - q0 < (long)ppt ? (int)(D.npair - q0) : ppt;   // 1 .. ppt pairs
        tn_key_t best = 0ull;   // of the pair's first lane
        float best_s = 0.0f;
        unsigned first = 0u, u = 0u;
        for (int t0 = 0; t0 < C; t0 += 64) {   // one turn when C <= 64
            const int cnt = C - t0 < 64 ? C - t0 : 64, live = np * cnt;   // lanes 0 .. live - 1 hold an entry
            const int pl = lane / cnt, li = lane - pl * cnt;
            const bool on = lane < live;
            unsigned cid = 0u;
            if (on) {
                const long q = q0 + pl;
                const long e = q * C + t0 + li;   // the plain rule's pair index: below 2^31 - 16
                u = D.user[(unsigned)q / (unsigned)D.num_neg];
                int took;
                if constexpr (WF == 0) took = pair_src_pick(D.seed, (uint64_t)e, D.num_item, D.uitems, D.uptr[u], D.uptr[u + 1], PAIR_SRC_DRAWS, &cid);
                else took = pair_weight_pick<WF>(D.seed, (uint64_t)e, T, D.uitems, D.uptr[u], D.uptr[u + 1], PAIR_SRC_DRAWS, &cid);
                if (!took) *D.flag = (unsigned)(e + 1);
            }
            float s = 0.0f;
            if constexpr (SUB == 0) {
                if (on) s = re_row_score(P.k, re_user_row(P, u), re_item_row(ibase, P.pitch, cid), ibias[cid]);
            } else {
                const int nch = P.pitch >> 2, nfull = P.k >> 2, ntail = P.k & 3;
                const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float bias = on ? ibias[cid] : 0.0f;
                const float4 *urow = re_user_row(P, u);   // (a lane without an entry does not read it)
                for (int r0 = 0; r0 < live; r0 += SUB) {
                    const int rows = live - r0 < SUB ? live - r0 : SUB, nel = rows * nch;
                    tn_wave_sync();   // the previous turn has been read (first trip: nothing yet)
                    for (int e0 = 0; e0 < nel; e0 += 64 * PH_NB) {   // every lane takes every trip: the shuffle reads lanes that stage nothing
                        float4 v[PH_NB];
                        int dst[PH_NB];
#pragma unroll
                        for (int b = 0; b < PH_NB; b++) {             // PH_NB requests ahead of their LDS stores
                            const int x = e0 + 64 * b + lane;
                            const bool in = x < nel;                  // a row past the turn's end is not loaded
                            const int row = in ? x / nch : 0, ch = x - row * nch;
                            const int item = __shfl((int)cid, r0 + row);
                            v[b] = zero4;
                            if (in) v[b] = re_item_row(ibase, P.pitch, item)[ch];
                            dst[b] = in ? ch * (SUB + 1) + row : -1;   // row < SUB, ch < nch: inside [nch][SUB + 1]
                        }
#pragma unroll
                        for (int b = 0; b < PH_NB; b++)
                            if (dst[b] >= 0) ph_item[dst[b]] = v[b];
                    }
                    tn_wave_sync();
                    if (lane >= r0 && lane < r0 + rows) {     // ... nor scored
                        const int row = lane - r0;
                        float acc[4];
                        acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
                        for (int j = 0; j < nfull; j++) {
                            const float4 v = ph_item[(size_t)j * (SUB + 1) + row];
                            const float4 p = urow[j];
                            acc[0] = acc[0] + p.x * v.x;
                            acc[1] = acc[1] + p.y * v.y;
                            acc[2] = acc[2] + p.z * v.z;
                            acc[3] = acc[3] + p.w * v.w;
                        }
                        float4 vt = zero4, pt = zero4;
                        if (ntail) { vt = ph_item[(size_t)nfull * (SUB + 1) + row]; pt = urow[nfull]; }
                        float sum = (acc[0] + acc[2]) + (acc[1] + acc[3]);
                        if (ntail) {
                            sum = sum + pt.x * vt.x;
                            if (ntail > 1) sum = sum + pt.y * vt.y;
                            if (ntail > 2) sum = sum + pt.z * vt.z;
                        }
                        s = 0.0f + (bias + sum);
                    }
                }
            }
            // ---- the best key of every pair's cnt lanes, into its first lane: after the step with offset o, lane li holds the maximum over
            // [li, min(li + 2 o, cnt)).  Equal keys carry equal scores; a NaN is key 0 and never replaces anything.
            tn_key_t key = on && s == s ? tn_key(s, (int)cid) : 0ull;
            for (int o = 1; o < cnt; o <<= 1) {
                const tn_key_t key_o = __shfl_down(key, o);
                const float s_o = __shfl_down(s, o);
                if (li + o < cnt && key_o > key) { key = key_o; s = s_o; }
            }
            if (li == 0) {
                if (t0 == 0) { best = key; best_s = s; first = cid; }
                else if (key > best) { best = key; best_s = s; }
            }
        }
        const int pl = lane / cnt0;
        if (pl < np && lane == pl * cnt0) {   // the pair's first lane: key 0 = every candidate scored NaN, cand(q, 0) and its score stay
            const long q = q0 + pl;
            if (D.out_user) {
                D.out_user[q] = u;
                D.out_pos[q] = D.pos[(unsigned)q / (unsigned)D.num_neg];
            }
            D.out_neg[q] = best ? (unsigned)tn_key_id(best) : first;
            if (H.out_score) H.out_score[q] = best_s;
        }
    }
}

static int ph_sub(int pitch) { return pitch <= 64 ? 64 : pitch <= 128 ? 32 : 16; }

// The measured choice (profiles/r34_pair_hard.md: 20 M pairs, 10 K items, num_factor 32 / 64 / 128 / 256 x num_cand 2 / 4 / 8 / 16): the
// staged form where it beat the lane form by more than both spreads -- every measured num_cand at 32 floats, num_cand <= 4 at 64 and 128,
// num_cand 2 at 256 --, the lane form everywhere else, unmeasured cells included: a width takes the column of the next measured width above
// it, a num_cand above 16 the lane form.
int pair_hard_form(const DevParams &P, int form, int num_cand) {
    if (P.pitch > 256) return 1;   // no LDS tile holds the rows
    if (form == 1 || form == 2) return form;
    const int most = P.pitch <= 32 ? 16 : P.pitch <= 128 ? 4 : 2;   // the largest num_cand the staged form takes
    return num_cand <= most ? 2 : 1;
}

template <int SUB>
static void ph_launch(const DevParams &P, const PairHardDev &H, const PairWeightDev &T, int wf, dim3 grid, size_t lds, long nunit, hipStream_t st) {
    if (wf == 0) hipLaunchKernelGGL((k_pair_hard<SUB, 0>), grid, dim3(64), lds, st, P, H, nunit, T);
    else if (wf == 2) hipLaunchKernelGGL((k_pair_hard<SUB, 2>), grid, dim3(64), lds, st, P, H, nunit, T);
    else hipLaunchKernelGGL((k_pair_hard<SUB, 1>), grid, dim3(64), lds, st, P, H, nunit, T);
}

void launch_pair_hard(const DevParams &P, const PairHardDev &H, const PairWeightDev &T, int wform, int form, hipStream_t st) {
    if (H.D.npair <= 0) return;
    const int wf = T.cdf ? pair_weight_form((long)T.num_item, wform) : 0;
    const int ppt = H.num_cand < 64 ? 64 / H.num_cand : 1;
    const long nunit = (H.D.npair + ppt - 1) / ppt;
    const dim3 grid((unsigned)std::min<long>(nunit, PH_MAX_GRID));
    if (pair_hard_form(P, form, H.num_cand) == 2) {
        const int sub = ph_sub(P.pitch);
        const size_t lds = 16 * ((size_t)P.pitch >> 2) * ((size_t)sub + 1);
        if (sub == 64) ph_launch<64>(P, H, T, wf, grid, lds, nunit, st);
        else if (sub == 32) ph_launch<32>(P, H, T, wf, grid, lds, nunit, st);
        else ph_launch<16>(P, H, T, wf, grid, lds, nunit, st);
    } else {
        ph_launch<0>(P, H, T, wf, grid, 0, nunit, st);
    }
}

}  // namespace svdf

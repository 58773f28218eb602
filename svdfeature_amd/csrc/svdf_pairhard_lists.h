// svdf_pairhard_lists.h -- the host-only part of the hard pass of a pair source (svdf_pair_hard_negatives / svdf_*_pair_source*_hard,
// DESIGN.md section 6ad): per pair, num_cand candidates of the plain rule (svdf_pairsource_lists.h) scored with the live model, the best
// of them by rank key the pair's negative.  The rule is stated in full in include/svdfeature_amd.h.  Here: the validation of a hard pass,
// the score in the ranker's pinned fp32 order (svdf_k_rankscore.h's re_row_score restated for the host -- build with -ffp-contract=off),
// the rank key of svdf_k_rankkey.h as plain integer code, and the sequential loop.  Plain C++ without a device call, so that
// tools/check_pairhard_lists.cpp can run it under a sanitizer.
#ifndef SVDF_PAIRHARD_LISTS_H_
#define SVDF_PAIRHARD_LISTS_H_

#include <cstring>

#include "svdf_pairweight_lists.h"

namespace svdf {

constexpr int PAIR_HARD_MAX_CAND = 256;   // largest num_cand; num_neg * num_cand stays within PAIR_SRC_MAX_NEG

// what a hard pass refuses about num_neg and num_cand: the expanded plain pass (num_neg * num_cand negatives per row) must be one
static inline void pair_hard_check_pass(long n, int num_neg, int num_cand) {
    if (num_neg < 1 || num_neg > PAIR_SRC_MAX_NEG) fail("pair_source: num_neg must be between 1 and 256");
    if (num_cand < 1 || num_cand > PAIR_HARD_MAX_CAND) fail("pair_source: num_cand must be between 1 and 256");
    if (num_neg * num_cand > PAIR_SRC_MAX_NEG) fail("pair_source: num_neg * num_cand must be at most 256");
    if (n * (long)(num_neg * num_cand) >= 0x7FFFFFF0L) fail("pair_source: n * num_neg * num_cand must stay below 2^31 - 16");
    pair_src_check_pass(n, num_neg * num_cand);
}

// i_bias + <p, v> as svdf_rank_topn scores it: four serial chains over the 4-float chunks, (a0 + a2) + (a1 + a3), the scalar tail,
// 0 + (bias + sum), every multiply and add rounded separately
static inline float pair_hard_score(int k, const float *p, const float *v, float bias) {
    const int nfull = k >> 2, ntail = k & 3;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int j = 0; j < nfull; j++) {
        a0 = a0 + p[4 * j] * v[4 * j]; a1 = a1 + p[4 * j + 1] * v[4 * j + 1];
        a2 = a2 + p[4 * j + 2] * v[4 * j + 2]; a3 = a3 + p[4 * j + 3] * v[4 * j + 3];
    }
    float sum = (a0 + a2) + (a1 + a3);
    for (int t = 0; t < ntail; t++) sum = sum + p[4 * nfull + t] * v[4 * nfull + t];
    return 0.0f + (bias + sum);
}

// tn_key(score, id) of svdf_k_rankkey.h: a larger key is a higher score, then a smaller id; -0 counts as +0; 0 stands for a NaN score
static inline uint64_t pair_hard_key(float s, unsigned id) {
    if (s != s) return 0;
    uint32_t b;
    std::memcpy(&b, &s, sizeof(b));
    if (b == 0x80000000u) b = 0u;
    const uint32_t w = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)w << 32) | (uint64_t)(uint32_t)~id;
}

// The sequential loop: pair q = r * num_neg + j takes the best of cand(q, 0 .. num_cand - 1), cand(q, i) the plain rule's negative of pair
// index q * num_cand + i.  neg_out[n * num_neg]; score_out (or nullptr) the chosen candidate's score.  An exhausted entry names its
// plain-rule pair index.  wt with a table: the candidates are the WEIGHTED plain rule's (section 6ae), in form wform (equal results).
static inline void pair_hard_draw_host(const PairSrcLists &L, long num_item, long n, const unsigned *user, int num_neg, int num_cand, uint64_t seed,
                                       int k, const float *W_user, const float *W_item, const float *i_bias, unsigned *neg_out, float *score_out,
                                       int max_draws = PAIR_SRC_DRAWS, const PairWeightDev *wt = nullptr, int wform = 1) {
    if (!neg_out || !W_user || !W_item || !i_bias || k < 1) fail("pair_source: bad arguments");
    for (long r = 0; r < n; r++) {
        const int p0 = L.uptr[user[r]], p1 = L.uptr[(size_t)user[r] + 1];
        const float *urow = W_user + (size_t)user[r] * (size_t)k;
        for (int j = 0; j < num_neg; j++) {
            const long q = r * num_neg + j;
            uint64_t best = 0;
            unsigned chosen = 0;
            float chosen_score = 0.0f;
            for (int i = 0; i < num_cand; i++) {
                const long e = q * num_cand + i;
                unsigned id;
                if (!pair_any_pick(seed, (uint64_t)e, (unsigned)num_item, L.uitems.data(), p0, p1, max_draws, &id, wt, wform))
                    fail("pair_source: pair " + std::to_string(e) + " found no negative in " + std::to_string(max_draws) + " draws");
                const float s = pair_hard_score(k, urow, W_item + (size_t)id * (size_t)k, i_bias[id]);
                const uint64_t key = pair_hard_key(s, id);
                if (i == 0 || key > best) { best = key; chosen = id; chosen_score = s; }   // (all NaN: every key is 0 and cand(q, 0) stays)
            }
            neg_out[q] = chosen;
            if (score_out) score_out[q] = chosen_score;
        }
    }
}

// svdf_pair_hard_negatives (item_weight == nullptr) and svdf_pair_hard_negatives_weighted: the whole rule on the host
static inline void pair_hard_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, int num_cand,
                                       uint64_t seed, int num_factor, const float *W_user, const float *W_item, const float *i_bias, unsigned *neg_out,
                                       float *score_out, const unsigned *item_weight = nullptr) {
    pair_src_check_rows(num_user, num_item, n, user, pos_item);
    pair_hard_check_pass(n, num_neg, num_cand);
    if (num_factor < 1 || num_factor > 1024) fail("pair_source: hard negatives need num_factor between 1 and 1024");
    PairSrcLists L;
    if (!item_weight) {
        pair_src_build(num_user, num_item, n, user, pos_item, L, pair_src_threads(n));
        pair_hard_draw_host(L, num_item, n, user, num_neg, num_cand, seed, num_factor, W_user, W_item, i_bias, neg_out, score_out);
        return;
    }
    PairWeightLists Wt;
    pair_weight_source(num_user, num_item, n, user, pos_item, item_weight, L, Wt);
    const PairWeightDev T = Wt.view();
    pair_hard_draw_host(L, num_item, n, user, num_neg, num_cand, seed, num_factor, W_user, W_item, i_bias, neg_out, score_out, PAIR_SRC_DRAWS, &T, 1);
}

}  // namespace svdf
#endif

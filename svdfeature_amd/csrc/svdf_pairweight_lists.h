// svdf_pairweight_lists.h -- the host-only part of ITEM-WEIGHTED negatives for the pair source (svdf_pair_source_create_weighted /
// svdf_pair_negatives_weighted / svdf_pair_weight_lookup): the map from a 64-bit random word onto an item id under a
// table of uint32 weights (stated in full in include/svdfeature_amd.h; the streams, mix and G are sections 6ab / 6ac's), the two tables the
// map reads (the running sums `cdf` and the guide table), the validation of the weights, the weighted density rule and the sequential
// draw loop.  Plain C++ without a device call, so that tools/check_pairweight_lists.cpp can run it under a sanitizer; the functions marked
// host / device are what k_pair_draw and k_pair_hard compute with when the source has weights.
#ifndef SVDF_PAIRWEIGHT_LISTS_H_
#define SVDF_PAIRWEIGHT_LISTS_H_

#include "svdf_pairsource_lists.h"

namespace svdf {

constexpr int PAIR_WEIGHT_MIN_GUIDE = 64;   // the guide table has at least this many buckets

// What a draw reads of a weight table.  cdf == nullptr: no weights (the uniform rule of section 6ac).
struct PairWeightDev {
    const unsigned *cdf = nullptr;     // [num_item + 1] cdf[0] = 0, cdf[i + 1] = cdf[i] + item_weight[i]; cdf[num_item] = W
    const unsigned *guide = nullptr;   // [Gn + 1] guide[g] = the item holding y = mulhi(g << shift, W); guide[Gn] = the last item of positive weight
    unsigned W = 0;                    // 1 .. 2^32 - 1
    unsigned num_item = 0;
    int shift = 0;                     // 64 - log2 Gn, Gn the smallest power of two >= max(num_item, 64): 33 .. 58
};

// floor(x * w / 2^64)
SVDF_RANK_NEGS_HD static inline uint64_t pair_weight_mulhi(uint64_t x, uint64_t w) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(x, w);
#else
    return (uint64_t)(((unsigned __int128)x * (unsigned __int128)w) >> 64);
#endif
}
// the largest i in [lo, hi] with cdf[i] <= y, for cdf[lo] <= y: then cdf[i + 1] > y wherever hi is at least the item that holds y
SVDF_RANK_NEGS_HD static inline unsigned pair_weight_search(const unsigned *cdf, unsigned lo, unsigned hi, unsigned y) {
    while (lo < hi) {
        const unsigned m = lo + ((hi - lo + 1u) >> 1);
        if (cdf[m] <= y) lo = m; else hi = m - 1u;
    }
    return lo;
}
// THE MAP: the item i with cdf[i] <= y < cdf[i + 1], y = mulhi(x, W) -- never an item of weight 0.  FORM 1 searches the whole cdf; FORM 2
// reads the guide entries of x's bucket and searches between them, both ends included: x >= g << shift gives y >= y_g, so the item is at or
// past guide[g]; x < (g + 1) << shift gives y <= y_(g + 1), so it is at or before guide[g + 1] (for the last bucket: the last item of
// positive weight).  Equal results by construction.
template <int FORM>
SVDF_RANK_NEGS_HD static inline unsigned pair_weight_lookup(const PairWeightDev &T, uint64_t x) {
    const unsigned y = (unsigned)pair_weight_mulhi(x, (uint64_t)T.W);   // < W
    if (FORM == 2) {
        const uint64_t g = x >> T.shift;
        return pair_weight_search(T.cdf, T.guide[g], T.guide[g + 1], y);
    }
    return pair_weight_search(T.cdf, 0u, T.num_item - 1u, y);
}
// draw t of a pair's stream under a weight table: all 64 bits of the mixed counter
template <int FORM>
SVDF_RANK_NEGS_HD static inline unsigned pair_weight_draw(uint64_t stream, uint64_t t, const PairWeightDev &T) {
    return pair_weight_lookup<FORM>(T, rank_negs_mix(stream + (t + 1) * RANK_NEGS_G));
}
// pair_src_pick under a weight table: the first of wdraw(q, 0), wdraw(q, 1), .. outside items[p0, p1), among at most max_draws.  Returns the
// draws taken, 0 when none of them was accepted (*neg is then 0).
template <int FORM>
SVDF_RANK_NEGS_HD static inline int pair_weight_pick(uint64_t seed, uint64_t q, const PairWeightDev &T, const unsigned *items, int p0, int p1, int max_draws,
                                                     unsigned *neg) {
    const uint64_t stream = pair_src_stream(seed, q);
    for (int t = 0; t < max_draws; t++) {
        const unsigned id = pair_weight_draw<FORM>(stream, (uint64_t)t, T);
        if (!pair_src_listed(items, p0, p1, id)) { *neg = id; return t + 1; }
    }
    *neg = 0u;
    return 0;
}
// the pick of a pair on the host, with or without a table: wt == nullptr (or one without cdf) is pair_src_pick
static inline int pair_any_pick(uint64_t seed, uint64_t q, unsigned num_item, const unsigned *items, int p0, int p1, int max_draws, unsigned *neg,
                                const PairWeightDev *wt, int form) {
    if (!wt || !wt->cdf) return pair_src_pick(seed, q, num_item, items, p0, p1, max_draws, neg);
    return form == 2 ? pair_weight_pick<2>(seed, q, *wt, items, p0, p1, max_draws, neg) : pair_weight_pick<1>(seed, q, *wt, items, p0, p1, max_draws, neg);
}

struct PairWeightLists {
    std::vector<unsigned> cdf, guide;
    int shift = 0;
    PairWeightDev view() const {
        PairWeightDev T;
        T.cdf = cdf.data(); T.guide = guide.data(); T.W = cdf.back(); T.num_item = (unsigned)(cdf.size() - 1); T.shift = shift;
        return T;
    }
};

// What a weighted source refuses about its weights, then both tables: the running sums, and the guide table in ONE pass over them (the
// bucket boundaries y_g ascend with g, so the item that holds them only moves forward).
static inline void pair_weight_build(long num_item, const unsigned *item_weight, PairWeightLists &out) {
    if (!item_weight || num_item < 1 || num_item > 0x7fffffffL) fail("pair_source: bad arguments");
    uint64_t sum = 0;
    for (long i = 0; i < num_item; i++) sum += item_weight[i];   // (below 2^63)
    if (sum == 0) fail("pair_source: the item weights sum to 0");
    if (sum > 0xFFFFFFFFull) fail("pair_source: the item weights sum to " + std::to_string(sum) + ": the sum must stay below 2^32");
    out.cdf.resize((size_t)num_item + 1);
    out.cdf[0] = 0u;
    long last = 0;
    for (long i = 0; i < num_item; i++) {
        out.cdf[(size_t)i + 1] = out.cdf[(size_t)i] + item_weight[i];
        if (item_weight[i]) last = i;
    }
    int lg = 6;   // log2 Gn
    while (((long)1 << lg) < num_item) lg++;
    const long Gn = (long)1 << lg;
    out.shift = 64 - lg;
    out.guide.resize((size_t)Gn + 1);
    long i = 0;
    for (long g = 0; g < Gn; g++) {
        const unsigned y = (unsigned)pair_weight_mulhi((uint64_t)g << out.shift, sum);   // < W = cdf[num_item]: the walk ends at or before `last`
        while (out.cdf[(size_t)i + 1] <= y) i++;
        out.guide[(size_t)g] = (unsigned)i;
    }
    out.guide[(size_t)Gn] = (unsigned)last;
}

// THE DENSITY RULE, WEIGHTED, in 64-bit integers: a user with rows must leave 64 * (W - W(P(u))) >= W, W(P(u)) the weight of its distinct
// items, so that every draw of every pair is accepted with probability >= 1 / 64 less the map's bias (the first such user in id order is
// named).  It replaces the count rule of pair_src_build: what matters to a weighted draw is the weight a user holds, not how many items.
static inline void pair_weight_density(long num_user, const PairSrcLists &L, const unsigned *item_weight, uint64_t W) {
    for (long u = 0; u < num_user; u++) {
        if (L.uptr[(size_t)u + 1] == L.uptr[(size_t)u]) continue;
        uint64_t held = 0;
        for (int p = L.uptr[(size_t)u]; p < L.uptr[(size_t)u + 1]; p++) held += item_weight[L.uitems[(size_t)p]];
        if (64 * (W - held) < W)
            fail("pair_source: user " + std::to_string(u) + "'s positive items hold " + std::to_string(held) + " of the total item weight " + std::to_string(W) +
                 ": less than 1 part in 64 is left to draw a negative from; draw its negatives yourself (svdf_dataset_from_pairs)");
    }
}

// everything a weighted source validates and builds on the host, in the order of its refusals: the rows, the weights, the density rule
static inline void pair_weight_source(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight,
                                      PairSrcLists &L, PairWeightLists &Wt) {
    pair_src_check_rows(num_user, num_item, n, user, pos_item);
    pair_weight_build(num_item, item_weight, Wt);
    pair_src_build(num_user, num_item, n, user, pos_item, L, pair_src_threads(n), false);
    pair_weight_density(num_user, L, item_weight, (uint64_t)Wt.cdf.back());
}

// The sequential draw loop under a weight table, in form 1 or 2 (equal results).  A pair that exhausts max_draws fails the call and names q.
static inline void pair_weight_draw_host(const PairSrcLists &L, const PairWeightDev &T, int form, long n, const unsigned *user, int num_neg, uint64_t seed,
                                         unsigned *neg_out, int max_draws = PAIR_SRC_DRAWS) {
    if (!neg_out) fail("pair_source: bad arguments");
    for (long r = 0; r < n; r++) {
        const int p0 = L.uptr[user[r]], p1 = L.uptr[(size_t)user[r] + 1];
        for (int j = 0; j < num_neg; j++) {
            const long q = r * num_neg + j;
            if (!pair_any_pick(seed, (uint64_t)q, T.num_item, L.uitems.data(), p0, p1, max_draws, neg_out + q, &T, form))
                fail("pair_source: pair " + std::to_string(q) + " found no negative in " + std::to_string(max_draws) + " draws");
        }
    }
}

// svdf_pair_negatives_weighted: the whole rule on the host
static inline void pair_weight_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight,
                                         int num_neg, uint64_t seed, unsigned *neg_out) {
    pair_src_check_rows(num_user, num_item, n, user, pos_item);
    pair_src_check_pass(n, num_neg);
    PairSrcLists L;
    PairWeightLists Wt;
    pair_weight_source(num_user, num_item, n, user, pos_item, item_weight, L, Wt);
    pair_weight_draw_host(L, Wt.view(), 1, n, user, num_neg, seed, neg_out);
}

// svdf_pair_weight_lookup on the host: the ids of the words x[0 .. nx) in form 1 or 2
static inline void pair_weight_lookup_host(const PairWeightDev &T, int form, long nx, const uint64_t *x, unsigned *id_out) {
    for (long j = 0; j < nx; j++) id_out[j] = form == 2 ? pair_weight_lookup<2>(T, x[j]) : pair_weight_lookup<1>(T, x[j]);
}

}  // namespace svdf
#endif

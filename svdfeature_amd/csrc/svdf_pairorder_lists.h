// svdf_pairorder_lists.h -- the host-only part of the shuffled pass of a pair source (svdf_pair_order / svdf_*_pair_source*_shuffled, DESIGN.md
// section 6af): the keyed bijection sigma on [0, n) that gives position p of a shuffled pass its source row -- a 4-round unbalanced Feistel
// network over b bits, walked until it lands below n.  The rule is stated in full in include/svdfeature_amd.h; mix and G are section 6ab's
// (svdf_ranknegs_lists.h).  Plain C++ without a device call, so that tools/check_pairorder_lists.cpp can run it under a sanitizer; the
// functions marked host / device are what k_pair_order computes with.
#ifndef SVDF_PAIRORDER_LISTS_H_
#define SVDF_PAIRORDER_LISTS_H_

#include "svdf_ranknegs_lists.h"

namespace svdf {

constexpr uint64_t PAIR_ORDER_SALT = 0x706169726F726472ull;   // ASCII "pairordr": order_seed and seed may be equal and stay independent
constexpr int PAIR_ORDER_WALKS = 128;                         // the applications of E a position may take

struct PairOrderKeys {
    uint64_t k[4];   // K_0 .. K_3
    int bits;        // b: the smallest integer >= 2 with 2^b >= n
};

SVDF_RANK_NEGS_HD static inline PairOrderKeys pair_order_keys(uint64_t order_seed, long n) {
    PairOrderKeys K;
    for (int i = 0; i < 4; i++) K.k[i] = rank_negs_mix((order_seed ^ PAIR_ORDER_SALT) + (uint64_t)(i + 1) * RANK_NEGS_G);
    K.bits = 2;
    while (((uint64_t)1 << K.bits) < (uint64_t)n) K.bits++;
    return K;
}

// E: one pass of the network over [0, 2^b), a bijection on it.  The halves trade widths every round; after four they are the first ones again.
SVDF_RANK_NEGS_HD static inline uint64_t pair_order_step(const PairOrderKeys &K, uint64_t x) {
    int wl = K.bits >> 1, wr = K.bits - wl;
    uint64_t L = x >> wr, R = x & (((uint64_t)1 << wr) - 1);
    for (int i = 0; i < 4; i++) {
        const uint64_t f = rank_negs_mix(K.k[i] + (R + 1) * RANK_NEGS_G) >> (64 - wl);   // (1 <= wl <= 16)
        const uint64_t l = L;
        L = R; R = l ^ f;
        const int w = wl; wl = wr; wr = w;
    }
    return (L << wr) | R;
}

// sigma(p): x = p, then x = E(x) until x < n -- at least one application, at most max_walks.  Returns the applications taken, 0 when they
// were exhausted (*row is then 0).
SVDF_RANK_NEGS_HD static inline int pair_order_sigma(const PairOrderKeys &K, long n, long p, int max_walks, unsigned *row) {
    uint64_t x = (uint64_t)p;
    for (int t = 1; t <= max_walks; t++) {
        x = pair_order_step(K, x);
        if (x < (uint64_t)n) { *row = (unsigned)x; return t; }
    }
    *row = 0u;
    return 0;
}

// what svdf_pair_order refuses about n, in the source's words
static inline void pair_order_check(long n) {
    if (n < 1) fail("pair_source: a source needs at least one row (n >= 1)");
    if (n >= 0x7FFFFFF0L) fail("pair_source: n * num_neg must stay below 2^31 - 16");
}

static inline std::string pair_order_spent(uint64_t order_seed, long p, int max_walks = PAIR_ORDER_WALKS) {
    return "pair_source: order_seed " + std::to_string(order_seed) + " needs more than " + std::to_string(max_walks) + " steps at position " +
           std::to_string(p) + "; take another order_seed";
}

// The sequential loop: sigma_out[n].  A position that exhausts max_walks fails the call and names itself.
static inline void pair_order_host(long n, uint64_t order_seed, unsigned *sigma_out, int max_walks = PAIR_ORDER_WALKS) {
    pair_order_check(n);
    if (!sigma_out) fail("pair_source: bad arguments");
    const PairOrderKeys K = pair_order_keys(order_seed, n);
    for (long p = 0; p < n; p++)
        if (!pair_order_sigma(K, n, p, max_walks, sigma_out + p)) fail(pair_order_spent(order_seed, p, max_walks));
}

// adjacent positions of the permuted order that share their user: what a source's `same` is for the caller's order
static inline long pair_order_same(long n, const unsigned *user, const unsigned *sigma) {
    long same = 0;
    for (long p = 1; p < n; p++) same += user[sigma[p]] == user[sigma[p - 1]];
    return same;
}

}  // namespace svdf
#endif

// svdf_pairsource_lists.h -- the host-only part of the pair source (svdf_pair_source_* / svdf_pair_negatives): the rule
// that draws one negative per pair of a pass from a source of positives (stated in full in include/svdfeature_amd.h; mix, draw and G are
// section 6ab's, svdf_ranknegs_lists.h), the validation of the source and of a pass, every user's distinct items (ascending), the density rule
// and the sequential draw loop.  Plain C++ without a device call, so that tools/check_pairsource_lists.cpp can run it under a sanitizer; the
// functions marked host / device are what k_pair_draw computes with.
#ifndef SVDF_PAIRSOURCE_LISTS_H_
#define SVDF_PAIRSOURCE_LISTS_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "svdf_ranknegs_lists.h"

namespace svdf {

constexpr uint64_t PAIR_SRC_SALT = 0x70616972736E6567ull;   // ASCII "pairsneg": a pass and a sampled= evaluation with one seed draw from different streams
constexpr int PAIR_SRC_DRAWS = 4096;                        // T: the draws a pair may take
constexpr int PAIR_SRC_MAX_NEG = 256;                       // largest num_neg
constexpr long PAIR_SRC_THREAD_ROWS = 1L << 18;             // sources above this many rows build their lists on several threads

// the stream of pair q = r * num_neg + j of a pass
SVDF_RANK_NEGS_HD static inline uint64_t pair_src_stream(uint64_t seed, uint64_t q) { return rank_negs_mix((seed ^ PAIR_SRC_SALT) + (q + 1) * RANK_NEGS_G); }
// whether `id` is among items[p0, p1), distinct and ascending
SVDF_RANK_NEGS_HD static inline bool pair_src_listed(const unsigned *items, int p0, int p1, unsigned id) {
    int lo = p0, hi = p1;
    while (lo < hi) {
        const int m = lo + ((hi - lo) >> 1);
        if (items[m] < id) lo = m + 1; else hi = m;
    }
    return lo < p1 && items[lo] == id;
}
// The negative of pair q: the first of draw(q, 0), draw(q, 1), .. outside items[p0, p1), among at most max_draws.  Returns the draws taken,
// 0 when none of them was accepted (*neg is then 0).
SVDF_RANK_NEGS_HD static inline int pair_src_pick(uint64_t seed, uint64_t q, unsigned num_item, const unsigned *items, int p0, int p1, int max_draws, unsigned *neg) {
    const uint64_t stream = pair_src_stream(seed, q);
    for (int t = 0; t < max_draws; t++) {
        const unsigned id = rank_negs_draw(stream, (uint64_t)t, num_item);
        if (!pair_src_listed(items, p0, p1, id)) { *neg = id; return t + 1; }
    }
    *neg = 0u;
    return 0;
}

struct PairSrcLists {
    std::vector<int> uptr;          // [num_user + 1] P(u) = uitems[uptr[u] .. uptr[u + 1]): the distinct items of all rows of user u, ascending
    std::vector<unsigned> uitems;
};

// what a source refuses about its rows, in svdf_dataset_from_pairs' words and order (row by row, the user first)
static inline void pair_src_check_rows(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item) {
    if (n < 1) fail("pair_source: a source needs at least one row (n >= 1)");
    if (!user || !pos_item || num_user < 1 || num_item < 1 || num_user > 0x7fffffffL || num_item > 0x7fffffffL) fail("pair_source: bad arguments");
    if (n >= 0x7FFFFFF0L) fail("pair_source: n * num_neg must stay below 2^31 - 16");
    for (long r = 0; r < n; r++) {
        if ((long)user[r] >= num_user) fail("user feature index exceed bound");
        if ((long)pos_item[r] >= num_item) fail("item feature index exceed bound");
    }
}
// what a pass refuses about num_neg
static inline void pair_src_check_pass(long n, int num_neg) {
    if (num_neg < 1 || num_neg > PAIR_SRC_MAX_NEG) fail("pair_source: num_neg must be between 1 and 256");
    if (n * (long)num_neg >= 0x7FFFFFF0L) fail("pair_source: n * num_neg must stay below 2^31 - 16");
}

// The lists of validated rows: a counting sort of the rows by user (a user's items in row order), then every user's slice sorted and its
// repeats dropped -- threads > 1: contiguous ranges of users with about equal numbers of rows side by side, the result that of one thread --,
// the slices closed up, and THE DENSITY RULE: a user with rows must leave 64 * (num_item - |P(u)|) >= num_item, so that every draw of
// every pair is accepted with probability >= 1 / 64 (the first such user in id order is named).  density = false leaves the rule out: a
// weighted source applies its own to the lists (svdf_pairweight_lists.h).
static inline void pair_src_build(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, PairSrcLists &out, int threads = 1,
                                  bool density = true) {
    std::vector<long> first((size_t)num_user + 1, 0);
    for (long r = 0; r < n; r++) first[(size_t)user[r] + 1]++;
    for (long u = 0; u < num_user; u++) first[(size_t)u + 1] += first[(size_t)u];
    std::vector<unsigned> raw((size_t)n);
    {
        std::vector<long> at(first.begin(), first.end() - 1);
        for (long r = 0; r < n; r++) raw[(size_t)at[user[r]]++] = pos_item[r];
    }
    std::vector<int> distinct((size_t)num_user, 0);
    auto range = [&](long a, long b) {
        for (long u = a; u < b; u++) {
            unsigned *p = raw.data() + first[(size_t)u], *e = raw.data() + first[(size_t)u + 1];
            std::sort(p, e);
            distinct[(size_t)u] = (int)(std::unique(p, e) - p);
        }
    };
    const int T = (int)std::max<long>(1, std::min<long>(threads, num_user));
    if (T == 1) range(0, num_user);
    else {
        std::vector<std::thread> th;
        long a = 0;
        for (int t = 1; t <= T; t++) {   // the first user whose rows start at or past n t / T
            const long b = t == T ? num_user : (long)(std::lower_bound(first.begin(), first.end() - 1, n * t / T) - first.begin());
            if (b > a) th.emplace_back(range, a, b);
            a = std::max(a, b);
        }
        for (std::thread &x : th) x.join();
    }
    out.uptr.assign((size_t)num_user + 1, 0);
    for (long u = 0; u < num_user; u++) {
        const long d = distinct[(size_t)u];
        if (density && d > 0 && 64 * (num_item - d) < num_item)
            fail("pair_source: user " + std::to_string(u) + " has " + std::to_string(d) + " distinct positive items of " + std::to_string(num_item) +
                 ": fewer than 1 item in 64 is left to draw a negative from; draw its negatives yourself (svdf_dataset_from_pairs)");
        out.uptr[(size_t)u + 1] = out.uptr[(size_t)u] + (int)d;
    }
    out.uitems.resize((size_t)out.uptr[(size_t)num_user]);
    for (long u = 0; u < num_user; u++)
        std::copy(raw.begin() + first[(size_t)u], raw.begin() + first[(size_t)u] + distinct[(size_t)u], out.uitems.begin() + out.uptr[(size_t)u]);
}

// The sequential draw loop: neg_out[n * num_neg], pair q = r * num_neg + j.  A pair that exhausts max_draws fails the call and names q.
static inline void pair_src_draw_host(const PairSrcLists &L, long num_item, long n, const unsigned *user, int num_neg, uint64_t seed, unsigned *neg_out,
                                      int max_draws = PAIR_SRC_DRAWS) {
    if (!neg_out) fail("pair_source: bad arguments");
    for (long r = 0; r < n; r++) {
        const int p0 = L.uptr[user[r]], p1 = L.uptr[(size_t)user[r] + 1];
        for (int j = 0; j < num_neg; j++) {
            const long q = r * num_neg + j;
            if (!pair_src_pick(seed, (uint64_t)q, (unsigned)num_item, L.uitems.data(), p0, p1, max_draws, neg_out + q))
                fail("pair_source: pair " + std::to_string(q) + " found no negative in " + std::to_string(max_draws) + " draws");
        }
    }
}

static inline int pair_src_threads(long n) {
    return n <= PAIR_SRC_THREAD_ROWS ? 1 : (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
}

// svdf_pair_negatives: the whole rule on the host
static inline void pair_src_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, uint64_t seed,
                                      unsigned *neg_out) {
    pair_src_check_rows(num_user, num_item, n, user, pos_item);
    pair_src_check_pass(n, num_neg);
    PairSrcLists L;
    pair_src_build(num_user, num_item, n, user, pos_item, L, pair_src_threads(n));
    pair_src_draw_host(L, num_item, n, user, num_neg, seed, neg_out);
}

}  // namespace svdf
#endif

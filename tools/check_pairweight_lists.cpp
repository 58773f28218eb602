// check_pairweight_lists.cpp -- the host-only part of item-weighted negatives for the pair source (svdfeature_amd/csrc/svdf_pairweight_lists.h:
// the map from a 64-bit word onto an item under a weight table in both forms, the running sums and the guide table, the validation of the
// weights, the weighted density rule, the sequential draw loop) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_pairweight_lists.cpp -o tools/check_pairweight_lists && tools/check_pairweight_lists
// The pinned vectors of the rule, both forms of the map against a linear scan on the boundary words of several tables (zero runs, one
// heavy item, a single positive item, W = 1 and W = 2^32 - 1), the guide table's entries, random sources against the definition over
// std::set, every refusal, the density rule at its edge, and the exhaustion of a pair's draws with a bound of 8.  Exit status 0 and "ok"
// when all holds.  With the argument "dump" it reads `num_user num_item n num_neg seed form`, then num_item weights, then n lines
// `user item` from standard input and prints the running sums, the guide table and the negatives: the form tests/test_pair_weight.py
// compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>

#include "svdf_pairweight_lists.h"

namespace svdf {
[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }
}  // namespace svdf

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

template <typename F>
static std::string refused(F f) {
    try { f(); } catch (const std::runtime_error &e) { return e.what(); }
    return "";
}

static std::vector<unsigned> pinned_weights(long ni) {
    std::vector<unsigned> w((size_t)ni);
    for (long i = 0; i < ni; i++) w[(size_t)i] = i % 7 == 0 ? 0u : 1u + (unsigned)((i * i) % 97);
    return w;
}

// the definition by a linear scan in 128-bit integers
static unsigned scan(const std::vector<unsigned> &w, uint64_t x) {
    unsigned __int128 W = 0;
    for (unsigned v : w) W += v;
    const unsigned __int128 y = ((unsigned __int128)x * W) >> 64;
    unsigned __int128 c = 0;
    for (size_t i = 0; i < w.size(); i++) {
        if (c <= y && y < c + w[i]) return (unsigned)i;
        c += w[i];
    }
    return ~0u;
}

// both forms on the boundary words of a table, and the guide table's own entries
static void check_table(const std::vector<unsigned> &w) {
    using namespace svdf;
    PairWeightLists Wt;
    EXPECT(refused([&] { pair_weight_build((long)w.size(), w.data(), Wt); }).empty());
    const PairWeightDev T = Wt.view();
    const uint64_t W = T.W;
    const long Gn = (long)Wt.guide.size() - 1;
    EXPECT(Wt.cdf.size() == w.size() + 1 && Gn >= 64 && Gn >= (long)w.size() && Gn < 2 * std::max<long>((long)w.size(), 64) && ((uint64_t)Gn << T.shift) == 0);
    std::vector<uint64_t> xs = {0, ~(uint64_t)0};
    for (size_t i = 0; i < w.size(); i++) {
        if (!w[i]) continue;
        const unsigned __int128 num = (unsigned __int128)Wt.cdf[i] << 64;
        const uint64_t x = (uint64_t)((num + W - 1) / W);   // the smallest word of item i
        xs.push_back(x);
        if (x) xs.push_back(x - 1);
    }
    for (long g = 0; g < Gn; g++) {
        xs.push_back((uint64_t)g << T.shift);
        xs.push_back((((uint64_t)g + 1) << T.shift) - 1);
        EXPECT(Wt.guide[(size_t)g] == scan(w, (uint64_t)g << T.shift));
    }
    long last = 0;
    for (size_t i = 0; i < w.size(); i++) if (w[i]) last = (long)i;
    EXPECT(Wt.guide[(size_t)Gn] == (unsigned)last);
    for (uint64_t x : xs) {
        const unsigned want = scan(w, x);
        EXPECT(want < w.size() && w[want] > 0);
        EXPECT(pair_weight_lookup<1>(T, x) == want);
        EXPECT(pair_weight_lookup<2>(T, x) == want);
    }
}

// negatives against the definition over std::set, both forms
static void check_source(long nu, long ni, const std::vector<unsigned> &user, const std::vector<unsigned> &pos, const std::vector<unsigned> &w, int num_neg,
                         uint64_t seed) {
    using namespace svdf;
    const long n = (long)user.size();
    std::vector<std::set<unsigned>> P((size_t)nu);
    for (long r = 0; r < n; r++) P[user[(size_t)r]].insert(pos[(size_t)r]);
    std::vector<unsigned> neg((size_t)n * (size_t)num_neg + 1, 0xDEADu);
    EXPECT(refused([&] { pair_weight_negatives(nu, ni, n, user.data(), pos.data(), w.data(), num_neg, seed, neg.data()); }).empty());
    EXPECT(neg.back() == 0xDEADu);
    PairSrcLists L;
    PairWeightLists Wt;
    pair_weight_source(nu, ni, n, user.data(), pos.data(), w.data(), L, Wt);
    std::vector<unsigned> neg2((size_t)n * (size_t)num_neg);
    pair_weight_draw_host(L, Wt.view(), 2, n, user.data(), num_neg, seed, neg2.data());
    for (long q = 0; q < n * num_neg; q++) {
        const std::set<unsigned> &mine = P[user[(size_t)(q / num_neg)]];
        const uint64_t stream = pair_src_stream(seed, (uint64_t)q);
        uint64_t t = 0;
        while (mine.count(scan(w, rank_negs_mix(stream + (t + 1) * RANK_NEGS_G)))) t++;
        const unsigned want = scan(w, rank_negs_mix(stream + (t + 1) * RANK_NEGS_G));
        EXPECT(neg[(size_t)q] == want && neg2[(size_t)q] == want && w[want] > 0 && t < (uint64_t)PAIR_SRC_DRAWS);
    }
}

static int dump() {
    using namespace svdf;
    long nu, ni, n;
    int num_neg, form;
    unsigned long long seed;
    if (std::scanf("%ld %ld %ld %d %llu %d", &nu, &ni, &n, &num_neg, &seed, &form) != 6) return 2;
    std::vector<unsigned> w((size_t)std::max<long>(ni, 0)), user((size_t)std::max<long>(n, 0)), pos(user.size());
    for (long i = 0; i < ni; i++)
        if (std::scanf("%u", &w[(size_t)i]) != 1) return 2;
    for (long r = 0; r < n; r++)
        if (std::scanf("%u %u", &user[(size_t)r], &pos[(size_t)r]) != 2) return 2;
    try {
        pair_src_check_rows(nu, ni, n, user.data(), pos.data());
        pair_src_check_pass(n, num_neg);
        PairSrcLists L;
        PairWeightLists Wt;
        pair_weight_source(nu, ni, n, user.data(), pos.data(), w.data(), L, Wt);
        std::vector<unsigned> neg((size_t)n * (size_t)num_neg);
        pair_weight_draw_host(L, Wt.view(), form, n, user.data(), num_neg, (uint64_t)seed, neg.data());
        auto line = [](const char *name, auto &v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); };
        line("cdf", Wt.cdf); line("guide", Wt.guide); line("neg", neg);
    } catch (const std::runtime_error &e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}

int main(int argc, char **argv) {
    using namespace svdf;
    if (argc > 1 && std::string(argv[1]) == "dump") return dump();
    // ---- the pinned vectors of the rule (include/svdfeature_amd.h)
    {
        const std::vector<unsigned> w = pinned_weights(1200);
        PairWeightLists Wt;
        pair_weight_build(1200, w.data(), Wt);
        const PairWeightDev T = Wt.view();
        EXPECT(T.W == 50185u && T.num_item == 1200u && T.shift == 64 - 11 && Wt.guide.size() == 2049);
        const unsigned d0[6] = {611, 1086, 472, 1016, 936, 514}, d7[8] = {502, 551, 33, 918, 200, 19, 1102, 177};
        for (int t = 0; t < 6; t++) EXPECT(pair_weight_draw<1>(pair_src_stream(12345, 0), (uint64_t)t, T) == d0[t] && pair_weight_draw<2>(pair_src_stream(12345, 0), (uint64_t)t, T) == d0[t]);
        for (int t = 0; t < 8; t++) EXPECT(pair_weight_draw<1>(pair_src_stream(12345, 7), (uint64_t)t, T) == d7[t] && pair_weight_draw<2>(pair_src_stream(12345, 7), (uint64_t)t, T) == d7[t]);
        const unsigned user[3] = {4, 4, 9}, pos[3] = {10, 700, 10};
        unsigned n1[3], n2[6];
        pair_weight_negatives(10, 1200, 3, user, pos, w.data(), 1, 12345, n1);
        pair_weight_negatives(10, 1200, 3, user, pos, w.data(), 2, 12345, n2);
        const unsigned w1[3] = {611, 547, 755}, w2[6] = {611, 547, 755, 1006, 59, 447};
        for (int j = 0; j < 3; j++) EXPECT(n1[j] == w1[j]);
        for (int j = 0; j < 6; j++) EXPECT(n2[j] == w2[j]);
        EXPECT(pair_weight_mulhi(~(uint64_t)0, 0xFFFFFFFFull) == 4294967294ull);
    }
    // ---- the map in both forms on the boundary words of its tables
    {
        check_table(pinned_weights(1200));
        for (long ni : {1L, 2L, 63L, 64L, 65L, 1200L, 5000L}) check_table(std::vector<unsigned>((size_t)ni, 1u));
        std::vector<unsigned> heavy(1200, 1u);
        heavy[417] = 0xFFFFFFFFu - 1199u;
        check_table(heavy);   // W = 2^32 - 1
        for (unsigned v : {1u, 0xFFFFFFFFu}) {
            std::vector<unsigned> one(300, 0u);
            one[123] = v;
            check_table(one);
        }
        std::vector<unsigned> z = pinned_weights(5000);
        for (size_t i = 0; i < 40; i++) z[i] = 0;
        for (size_t i = 4925; i < 5000; i++) z[i] = 0;
        for (size_t i = 2400; i < 2700; i++) z[i] = 0;
        check_table(z);
        std::vector<unsigned> run(500, 1000u);
        for (size_t i = 100; i < 300; i++) run[i] = 1u;
        run[300] = 1u << 31;
        check_table(run);
    }
    // ---- random sources: repeated rows, users without rows and with one, grouped and shuffled
    for (int num_neg : {1, 2, 7, 64}) {
        const long nu = 60, ni = 200, n = 900;
        std::mt19937 rng(31 + (unsigned)num_neg);
        std::vector<unsigned> user, pos, w((size_t)ni);
        for (long i = 0; i < ni; i++) w[(size_t)i] = i % 5 == 0 ? 0u : 1u + (unsigned)(rng() % 50);
        for (long r = 0; r < n; r++) {
            if (r > 10 && rng() % 6 == 0) { const size_t j = rng() % user.size(); user.push_back(user[j]); pos.push_back(pos[j]); continue; }
            user.push_back(3 + (unsigned)(rng() % (nu - 3)));
            pos.push_back((unsigned)(rng() % ni));
        }
        user[0] = 2;   // one row; users 0 and 1 have none
        check_source(nu, ni, user, pos, w, num_neg, 99);
        std::vector<size_t> at((size_t)n);
        for (size_t j = 0; j < at.size(); j++) at[j] = j;
        std::stable_sort(at.begin(), at.end(), [&](size_t a, size_t b) { return user[a] < user[b]; });
        std::vector<unsigned> gu, gp;
        for (size_t j : at) { gu.push_back(user[j]); gp.push_back(pos[j]); }
        check_source(nu, ni, gu, gp, w, num_neg, (uint64_t)1 << 63 | 5);
    }
    // ---- the weighted density rule at its edge, and the exhaustion of a pair's draws
    {
        // 128 items: item 0 weighs 6300 - 126, items 1 .. 126 weigh 1, item 127 weighs 100: the user of items 0 .. 126 holds 6300 of W = 6400
        const long ni = 128;
        std::vector<unsigned> w((size_t)ni, 1u), user(127, 0u), pos(127);
        w[0] = 6300u - 126u; w[127] = 100u;
        for (unsigned i = 0; i < 127; i++) pos[i] = i;
        PairSrcLists L;
        PairWeightLists Wt;
        EXPECT(refused([&] { pair_weight_source(2, ni, 127, user.data(), pos.data(), w.data(), L, Wt); }).empty());   // 64 * 100 == 6400
        std::vector<unsigned> neg(127 * 50);
        EXPECT(refused([&] { pair_weight_draw_host(L, Wt.view(), 2, 127, user.data(), 50, 7, neg.data()); }).empty());
        for (unsigned v : neg) EXPECT(v == 127);
        // a bound of 8 in place of T: some pair of the 6 350 needs more than 8 draws at acceptance 1 / 64
        for (int form : {1, 2}) {
            const std::string m = refused([&] { pair_weight_draw_host(L, Wt.view(), form, 127, user.data(), 50, 7, neg.data(), 8); });
            EXPECT(m.rfind("pair_source: pair ", 0) == 0 && m.find(" found no negative in 8 draws") != std::string::npos);
        }
        unsigned one = 77;
        EXPECT(pair_weight_pick<1>(7, 0, Wt.view(), L.uitems.data(), 0, 127, 0, &one) == 0 && one == 0);
        w[127] = 99u;   // one unit less is left
        EXPECT(refused([&] { pair_weight_source(2, ni, 127, user.data(), pos.data(), w.data(), L, Wt); }) ==
               "pair_source: user 0's positive items hold 6300 of the total item weight 6399: less than 1 part in 64 is left to draw a negative from; draw its "
               "negatives yourself (svdf_dataset_from_pairs)");
        // a user whose ONE popular positive holds more than 63 / 64 of W: the count rule (1 item of 128) would admit it
        const unsigned u1[1] = {1}, p1[1] = {0};
        std::vector<unsigned> pop((size_t)ni, 1u);
        pop[0] = 10000u;   // 64 * 127 < 10127
        PairSrcLists plain;
        EXPECT(refused([&] { pair_src_build(2, ni, 1, u1, p1, plain); }).empty());
        EXPECT(refused([&] { pair_weight_source(2, ni, 1, u1, p1, pop.data(), L, Wt); }).rfind("pair_source: user 1's positive items hold 10000 of the total item weight 10127", 0) == 0);
    }
    // ---- refusals
    {
        const unsigned user[3] = {1, 2, 9}, pos[3] = {5, 6, 7}, pbad[3] = {5, 6, 30};
        std::vector<unsigned> w(30, 1u), zero(30, 0u), big(30, 0u);
        big[3] = 0xFFFFFFFFu; big[29] = 1u;
        unsigned out[3];
        PairWeightLists Wt;
        EXPECT(refused([&] { pair_weight_build(30, zero.data(), Wt); }) == "pair_source: the item weights sum to 0");
        EXPECT(refused([&] { pair_weight_build(30, big.data(), Wt); }) == "pair_source: the item weights sum to 4294967296: the sum must stay below 2^32");
        big[29] = 0u;
        EXPECT(refused([&] { pair_weight_build(30, big.data(), Wt); }).empty() && Wt.view().W == 0xFFFFFFFFu);
        EXPECT(refused([&] { pair_weight_build(30, nullptr, Wt); }) == "pair_source: bad arguments");
        EXPECT(refused([&] { pair_weight_negatives(10, 30, 3, user, pbad, zero.data(), 1, 1, out); }) == "item feature index exceed bound");   // the rows first
        EXPECT(refused([&] { pair_weight_negatives(10, 30, 3, user, pos, zero.data(), 0, 1, out); }) == "pair_source: num_neg must be between 1 and 256");
        EXPECT(refused([&] { pair_weight_negatives(10, 30, 3, user, pos, zero.data(), 1, 1, out); }) == "pair_source: the item weights sum to 0");
        EXPECT(refused([&] { pair_weight_negatives(10, 30, 3, user, pos, w.data(), 1, 1, nullptr); }) == "pair_source: bad arguments");
        EXPECT(refused([&] { pair_weight_negatives(10, 30, 3, user, pos, w.data(), 1, 1, out); }).empty());
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

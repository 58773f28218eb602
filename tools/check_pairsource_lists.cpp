// check_pairsource_lists.cpp -- the host-only part of the pair source (svdfeature_amd/csrc/svdf_pairsource_lists.h: the rule that draws a
// pair's negative, the validation of a source and of a pass, every user's distinct items, the density rule, the sequential draw loop) as a
// stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_pairsource_lists.cpp -o tools/check_pairsource_lists && tools/check_pairsource_lists
// The pinned vectors of the rule, random sources (repeated rows, users without rows, grouped and shuffled orders, lists built on several
// threads), every refusal, the density rule at its edge, and the exhaustion of a pair's draws with a tiny bound.  Exit status 0 and "ok"
// when all holds.  With the argument "dump" it reads `num_user num_item n num_neg seed`, then n lines `user item` from standard input and
// prints the list offsets, the lists and the negatives: the form tests/test_pair_source.py compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>

#include "svdf_pairsource_lists.h"

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

// lists and negatives against their definitions over std::set
static void check_source(long nu, long ni, const std::vector<unsigned> &user, const std::vector<unsigned> &pos, int num_neg, uint64_t seed) {
    using namespace svdf;
    const long n = (long)user.size();
    PairSrcLists L;
    EXPECT(refused([&] { pair_src_check_rows(nu, ni, n, user.data(), pos.data()); pair_src_build(nu, ni, n, user.data(), pos.data(), L); }).empty());
    std::vector<std::set<unsigned>> P((size_t)nu);
    for (long r = 0; r < n; r++) P[user[(size_t)r]].insert(pos[(size_t)r]);
    EXPECT((long)L.uptr.size() == nu + 1 && L.uptr[0] == 0 && (size_t)L.uptr[(size_t)nu] == L.uitems.size());
    for (long u = 0; u < nu; u++) {
        EXPECT(L.uptr[(size_t)u + 1] - L.uptr[(size_t)u] == (int)P[(size_t)u].size());
        int at = L.uptr[(size_t)u];
        for (unsigned c : P[(size_t)u]) { EXPECT(L.uitems[(size_t)at] == c); at++; }   // distinct, ascending
    }
    for (int threads : {2, 3, 16, 1000}) {
        PairSrcLists M;
        pair_src_build(nu, ni, n, user.data(), pos.data(), M, threads);
        EXPECT(M.uptr == L.uptr && M.uitems == L.uitems);
    }
    std::vector<unsigned> neg((size_t)n * (size_t)num_neg + 1, 0xDEADu);
    pair_src_negatives(nu, ni, n, user.data(), pos.data(), num_neg, seed, neg.data());
    EXPECT(neg.back() == 0xDEADu);
    for (long q = 0; q < n * num_neg; q++) {
        const std::set<unsigned> &mine = P[user[(size_t)(q / num_neg)]];
        const uint64_t stream = pair_src_stream(seed, (uint64_t)q);
        uint64_t t = 0;
        while (mine.count(rank_negs_draw(stream, t, (unsigned)ni))) t++;
        EXPECT(neg[(size_t)q] == rank_negs_draw(stream, t, (unsigned)ni) && (long)neg[(size_t)q] < ni && t < (uint64_t)PAIR_SRC_DRAWS);
    }
}

static int dump() {
    using namespace svdf;
    long nu, ni, n;
    int num_neg;
    unsigned long long seed;
    if (std::scanf("%ld %ld %ld %d %llu", &nu, &ni, &n, &num_neg, &seed) != 5) return 2;
    std::vector<unsigned> user((size_t)std::max<long>(n, 0)), pos(user.size());
    for (long r = 0; r < n; r++)
        if (std::scanf("%u %u", &user[(size_t)r], &pos[(size_t)r]) != 2) return 2;
    try {
        pair_src_check_rows(nu, ni, n, user.data(), pos.data());
        pair_src_check_pass(n, num_neg);
        PairSrcLists L;
        pair_src_build(nu, ni, n, user.data(), pos.data(), L, 3);
        std::vector<unsigned> neg((size_t)n * (size_t)num_neg);
        pair_src_draw_host(L, ni, n, user.data(), num_neg, (uint64_t)seed, neg.data());
        auto line = [](const char *name, auto &v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); };
        line("uptr", L.uptr); line("uitems", L.uitems); line("neg", neg);
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
        EXPECT(PAIR_SRC_SALT == 0x70616972736E6567ull);
        EXPECT(pair_src_stream(12345, 0) == 0x6df61f806828913eull && pair_src_stream(12345, 7) == 0x0cee3333c9e3d7d8ull);
        EXPECT(pair_src_stream(12345, 0) != rank_negs_stream(12345, 0));   // the salt separates the streams
        const unsigned d0[6] = {607, 1083, 476, 1017, 945, 510}, d7[8] = {496, 554, 32, 921, 199, 15, 1103, 184};
        for (int t = 0; t < 6; t++) EXPECT(rank_negs_draw(pair_src_stream(12345, 0), (uint64_t)t, 1200) == d0[t]);
        for (int t = 0; t < 8; t++) EXPECT(rank_negs_draw(pair_src_stream(12345, 7), (uint64_t)t, 1200) == d7[t]);
        const unsigned user[3] = {4, 4, 9}, pos[3] = {10, 700, 10};
        unsigned n1[3], n2[6];
        pair_src_negatives(10, 1200, 3, user, pos, 1, 12345, n1);
        pair_src_negatives(10, 1200, 3, user, pos, 2, 12345, n2);
        const unsigned w1[3] = {607, 549, 766}, w2[6] = {607, 549, 766, 1010, 64, 448};
        for (int j = 0; j < 3; j++) EXPECT(n1[j] == w1[j]);
        for (int j = 0; j < 6; j++) EXPECT(n2[j] == w2[j]);
        const unsigned pos607[3] = {10, 607, 10};
        pair_src_negatives(10, 1200, 3, user, pos607, 1, 12345, n1);
        EXPECT(n1[0] == 1083);   // 607 is the user's: the second draw
    }
    // ---- random sources: repeated rows, users without rows and with one, grouped and shuffled
    for (int num_neg : {1, 2, 5, 64}) {
        const long nu = 60, ni = 200, n = 900;
        std::mt19937 rng(31 + (unsigned)num_neg);
        std::vector<unsigned> user, pos;
        for (long r = 0; r < n; r++) {
            if (r > 10 && rng() % 6 == 0) { const size_t j = rng() % user.size(); user.push_back(user[j]); pos.push_back(pos[j]); continue; }
            user.push_back(3 + (unsigned)(rng() % (nu - 3)));
            pos.push_back((unsigned)(rng() % ni));
        }
        user[0] = 2;   // one row; users 0 and 1 have none
        check_source(nu, ni, user, pos, num_neg, 99);
        std::vector<size_t> at((size_t)n);
        for (size_t j = 0; j < at.size(); j++) at[j] = j;
        std::stable_sort(at.begin(), at.end(), [&](size_t a, size_t b) { return user[a] < user[b]; });
        std::vector<unsigned> gu, gp;
        for (size_t j : at) { gu.push_back(user[j]); gp.push_back(pos[j]); }
        check_source(nu, ni, gu, gp, num_neg, (uint64_t)1 << 63 | 5);
    }
    // ---- the density rule at its edge, and the exhaustion of a pair's draws
    {
        const long ni = 6400;
        std::vector<unsigned> user(6300, 0u), pos(6300);
        for (unsigned i = 0; i < 6300; i++) pos[i] = i;
        PairSrcLists L;
        EXPECT(refused([&] { pair_src_build(2, ni, 6300, user.data(), pos.data(), L); }).empty());   // 64 * 100 == 6400
        std::vector<unsigned> neg(6300);
        EXPECT(refused([&] { pair_src_draw_host(L, ni, 6300, user.data(), 1, 7, neg.data()); }).empty());
        for (unsigned v : neg) EXPECT(v >= 6300 && v < 6400);
        // a tiny bound in place of T: some pair of the 6 300 needs more than 8 draws at acceptance 1 / 64
        const std::string m = refused([&] { pair_src_draw_host(L, ni, 6300, user.data(), 1, 7, neg.data(), 8); });
        EXPECT(m.rfind("pair_source: pair ", 0) == 0 && m.find(" found no negative in 8 draws") != std::string::npos);
        unsigned one = 77;
        EXPECT(pair_src_pick(7, 0, (unsigned)ni, L.uitems.data(), 0, 6300, 0, &one) == 0 && one == 0);
        user.push_back(0); pos.push_back(6300);
        EXPECT(refused([&] { pair_src_build(2, ni, 6301, user.data(), pos.data(), L); }) ==
               "pair_source: user 0 has 6301 distinct positive items of 6400: fewer than 1 item in 64 is left to draw a negative from; draw its negatives "
               "yourself (svdf_dataset_from_pairs)");
        user.push_back(0); pos.push_back(5);   // a repeated item does not count twice
        EXPECT(refused([&] { pair_src_build(2, ni, 6300, user.data() + 2, pos.data() + 2, L); }).empty());
    }
    // ---- refusals
    {
        const unsigned user[3] = {1, 2, 9}, pos[3] = {5, 6, 7}, ubad[3] = {1, 10, 9}, pbad[3] = {5, 6, 30}, both[3] = {1, 10, 9};
        unsigned out[3];
        auto rows = [&](long n, const unsigned *u, const unsigned *p) { return refused([&] { pair_src_check_rows(10, 30, n, u, p); }); };
        EXPECT(rows(3, user, pos).empty());
        EXPECT(rows(0, user, pos) == "pair_source: a source needs at least one row (n >= 1)");
        EXPECT(rows(-1, user, pos) == "pair_source: a source needs at least one row (n >= 1)");
        EXPECT(rows(3, nullptr, pos) == "pair_source: bad arguments");
        EXPECT(rows(3, ubad, pos) == "user feature index exceed bound");
        EXPECT(rows(3, user, pbad) == "item feature index exceed bound");
        EXPECT(rows(3, both, pbad) == "user feature index exceed bound");   // row 1 comes before row 2
        EXPECT(refused([&] { pair_src_check_pass(3, 0); }) == "pair_source: num_neg must be between 1 and 256");
        EXPECT(refused([&] { pair_src_check_pass(3, 257); }) == "pair_source: num_neg must be between 1 and 256");
        EXPECT(refused([&] { pair_src_check_pass(3, 256); }).empty());
        EXPECT(refused([&] { pair_src_check_pass(((1L << 31) - 16) / 2, 2); }) == "pair_source: n * num_neg must stay below 2^31 - 16");
        EXPECT(refused([&] { pair_src_check_pass(((1L << 31) - 16) / 2 - 1, 2); }).empty());
        EXPECT(refused([&] { pair_src_negatives(10, 30, 3, user, pos, 1, 1, nullptr); }) == "pair_source: bad arguments");
        EXPECT(refused([&] { pair_src_negatives(10, 30, 3, user, pos, 1, 1, out); }).empty());
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

// check_pairorder_lists.cpp -- the host-only part of the shuffled pass of a pair source (svdfeature_amd/csrc/svdf_pairorder_lists.h: the keys,
// the network E, the walk sigma with its bound, the sequential loop) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_pairorder_lists.cpp -o tools/check_pairorder_lists && tools/check_pairorder_lists
// The pinned vectors of the rule, E a bijection on [0, 2^b) for every b up to 16, sigma a bijection on [0, n) for every n up to 3000 and at the
// sizes around the powers of two up to 2^17 + 1, the pinned pass on the permuted rows, the count of adjacent positions that share a user, the
// refusals, and the exhaustion of a walk with the bound lowered.  Exit status 0 and "ok" when all holds.  With the argument "dump" it reads
// `n order_seed max_walks` from standard input and prints `sigma ...` and `steps ...` (the applications of E every position took), or
// `refused MESSAGE`: the form tests/test_pair_order.py compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "svdf_pairorder_lists.h"
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

static std::vector<unsigned> sigma_of(long n, uint64_t order_seed) {
    std::vector<unsigned> s((size_t)n + 1, 0xDEADu);
    svdf::pair_order_host(n, order_seed, s.data());
    EXPECT(s.back() == 0xDEADu);
    s.pop_back();
    return s;
}

static bool is_permutation(const std::vector<unsigned> &s) {
    std::vector<char> seen(s.size(), 0);
    for (unsigned v : s) {
        if ((size_t)v >= s.size() || seen[v]) return false;
        seen[v] = 1;
    }
    return true;
}

static int dump() {
    using namespace svdf;
    long n;
    unsigned long long seed;
    int walks;
    if (std::scanf("%ld %llu %d", &n, &seed, &walks) != 3) return 2;
    if (walks < 1) return 2;
    try {
        pair_order_check(n);
        if (n > 10000000) return 2;
        std::vector<unsigned> s((size_t)n);
        std::vector<int> steps((size_t)n);
        const PairOrderKeys K = pair_order_keys((uint64_t)seed, n);
        for (long p = 0; p < n; p++) {
            steps[(size_t)p] = pair_order_sigma(K, n, p, walks, &s[(size_t)p]);
            if (!steps[(size_t)p]) fail(pair_order_spent((uint64_t)seed, p, walks));
        }
        std::vector<unsigned> loop((size_t)n);
        pair_order_host(n, (uint64_t)seed, loop.data(), walks);   // (the loop itself: the same columns)
        if (loop != s) return 3;
        std::printf("sigma");
        for (unsigned x : s) std::printf(" %u", x);
        std::printf("\nsteps");
        for (int x : steps) std::printf(" %d", x);
        std::printf("\n");
    } catch (const std::runtime_error &e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}

int main(int argc, char **argv) {
    using namespace svdf;
    if (argc > 1 && std::string(argv[1]) == "dump") return dump();
    // ---- the pinned vectors (include/svdfeature_amd.h)
    {
        const PairOrderKeys K = pair_order_keys(12345, 10);
        EXPECT(K.k[0] == 0x55f0c474c3817246ull && K.k[1] == 0x212e2874c5b74625ull && K.k[2] == 0x1b12a40bba019e32ull && K.k[3] == 0xdbe2e77f7d83df15ull);
        EXPECT(K.bits == 4);
        EXPECT(pair_order_keys(1, 1).bits == 2 && pair_order_keys(1, 4).bits == 2 && pair_order_keys(1, 5).bits == 3 && pair_order_keys(1, 8).bits == 3);
        EXPECT(pair_order_keys(1, 9).bits == 4 && pair_order_keys(1, 0x7FFFFFEFL).bits == 31);
        EXPECT((sigma_of(10, 12345) == std::vector<unsigned>{2, 4, 8, 3, 7, 1, 6, 9, 0, 5}));
        EXPECT((sigma_of(10, 12346) == std::vector<unsigned>{0, 8, 1, 6, 3, 9, 7, 5, 2, 4}));
        const std::vector<unsigned> big = sigma_of(1200, 12345);
        EXPECT((std::vector<unsigned>(big.begin(), big.begin() + 8) == std::vector<unsigned>{648, 161, 507, 552, 509, 792, 1082, 757}));
        EXPECT((sigma_of(3, 12345) == std::vector<unsigned>{1, 2, 0}) && (sigma_of(2, 12345) == std::vector<unsigned>{1, 0}));
        unsigned row = 7;
        EXPECT(pair_order_sigma(pair_order_keys(12345, 1), 1, 0, PAIR_ORDER_WALKS, &row) == 4 && row == 0);   // n = 1: after four applications
        // the pass on the permuted rows
        const unsigned user[3] = {4, 4, 9}, pos[3] = {10, 700, 10};
        const std::vector<unsigned> s = sigma_of(3, 12345);
        unsigned pu[3], pp[3], neg[3];
        for (int p = 0; p < 3; p++) { pu[p] = user[s[(size_t)p]]; pp[p] = pos[s[(size_t)p]]; }
        pair_src_negatives(10, 1200, 3, pu, pp, 1, 12345, neg);
        EXPECT(pu[0] == 4 && pp[0] == 700 && neg[0] == 607 && pu[1] == 9 && pp[1] == 10 && neg[1] == 549 && pu[2] == 4 && pp[2] == 10 && neg[2] == 766);
    }
    // ---- E is a bijection on [0, 2^b)
    for (int b = 2; b <= 16; b++) {
        const long n = 1L << b;
        const PairOrderKeys K = pair_order_keys(0x1234567ull * (uint64_t)b, n);
        EXPECT(K.bits == b);
        std::vector<unsigned> image((size_t)n);
        for (long x = 0; x < n; x++) image[(size_t)x] = (unsigned)pair_order_step(K, (uint64_t)x);
        EXPECT(is_permutation(image));
    }
    // ---- sigma is a bijection on [0, n): every small n, the sizes around the powers of two, four order seeds
    {
        const uint64_t seeds[4] = {0, 12345, (uint64_t)1 << 63 | 5, ~(uint64_t)0};
        int longest = 0;
        for (long n = 1; n <= 3000; n++) EXPECT(is_permutation(sigma_of(n, seeds[n & 3])));
        for (int k = 12; k <= 17; k++)
            for (long n : {(1L << k) - 1, 1L << k, (1L << k) + 1})
                for (uint64_t seed : seeds) {
                    EXPECT(is_permutation(sigma_of(n, seed)));
                    const PairOrderKeys K = pair_order_keys(seed, n);
                    unsigned row;
                    for (long p = 0; p < n; p++) longest = std::max(longest, pair_order_sigma(K, n, p, PAIR_ORDER_WALKS, &row));
                }
        EXPECT(longest >= 2 && longest < 64);
        EXPECT(sigma_of(10, 12345) != sigma_of(10, 12346));
    }
    // ---- the count of adjacent positions that share a user
    {
        std::vector<unsigned> user(4000);
        for (size_t r = 0; r < user.size(); r++) user[r] = (unsigned)(r * 300 / user.size());
        std::vector<unsigned> id(4000);
        for (size_t r = 0; r < id.size(); r++) id[r] = (unsigned)r;
        EXPECT(pair_order_same(4000, user.data(), id.data()) == 3700);
        const long after = pair_order_same(4000, user.data(), sigma_of(4000, 12345).data());
        EXPECT(2 * after < 4000 && after < 100);
        const unsigned one[1] = {0};
        EXPECT(pair_order_same(1, user.data(), one) == 0);
    }
    // ---- exhaustion with the bound lowered: the first position that needs more steps is named, in the published words
    {
        const long n = 1025;   // b = 11: about half of [0, 2^b) lies outside
        const PairOrderKeys K = pair_order_keys(12345, n);
        long first = -1;
        unsigned row;
        for (long p = 0; p < n && first < 0; p++)
            if (pair_order_sigma(K, n, p, PAIR_ORDER_WALKS, &row) > 2) first = p;
        EXPECT(first >= 0);
        std::vector<unsigned> s((size_t)n);
        EXPECT(refused([&] { pair_order_host(n, 12345, s.data(), 2); }) ==
               "pair_source: order_seed 12345 needs more than 2 steps at position " + std::to_string(first) + "; take another order_seed");
        EXPECT(pair_order_sigma(K, n, first, 2, &row) == 0 && row == 0);
        EXPECT(pair_order_spent(~(uint64_t)0, 7) == "pair_source: order_seed 18446744073709551615 needs more than 128 steps at position 7; take another order_seed");
    }
    // ---- refusals
    {
        unsigned out[4];
        EXPECT(refused([&] { pair_order_host(0, 1, out); }) == "pair_source: a source needs at least one row (n >= 1)");
        EXPECT(refused([&] { pair_order_host(-3, 1, out); }) == "pair_source: a source needs at least one row (n >= 1)");
        EXPECT(refused([&] { pair_order_host(0x7FFFFFF0L, 1, out); }) == "pair_source: n * num_neg must stay below 2^31 - 16");
        EXPECT(refused([&] { pair_order_host(4, 1, nullptr); }) == "pair_source: bad arguments");
        EXPECT(refused([&] { pair_order_host(4, 1, out); }).empty());
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

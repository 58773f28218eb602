// check_pairhard_lists.cpp -- the host-only part of the hard pass of a pair source (svdfeature_amd/csrc/svdf_pairhard_lists.h: the validation
// of a hard pass, the score in the ranker's float32 order, the rank key, the sequential loop that keeps the best of num_cand candidates) as a
// stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_pairhard_lists.cpp -o tools/check_pairhard_lists && tools/check_pairhard_lists
// The pinned vectors of the rule, random sources and models against the definition written out over the plain pass's negatives (num_cand 1,
// 2, 7, 64, 65, 100 and 256: below, at and above a wave's 64 lanes), ties, +-0, NaN and +-inf scores, every refusal, and the exhaustion of an
// entry's draws with a tiny bound.  Exit status 0 and "ok" when all holds.  With the argument "dump" it reads `num_user num_item n num_neg
// num_cand seed num_factor`, then n lines `user item`, then W_user, W_item and i_bias as hexadecimal float32 bit patterns from standard
// input and prints the negatives and the bit patterns of the chosen scores: the form tests/test_pair_hard.py compares with numpy.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>

#include "svdf_pairhard_lists.h"

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

static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

struct Model {
    long nu, ni;
    int k;
    std::vector<float> wu, wi, bias;
};

// the definition, over the plain pass's negatives: a higher score wins, equal scores (+0 == -0) go to the smaller id, a NaN never wins
static void check_hard(const Model &M, const std::vector<unsigned> &user, const std::vector<unsigned> &pos, int m, int C, uint64_t seed) {
    using namespace svdf;
    const long n = (long)user.size(), N = n * m;
    std::vector<unsigned> cand((size_t)N * (size_t)C), neg((size_t)N + 1, 0xDEADu);
    std::vector<float> score((size_t)N + 1, -77.0f);
    pair_src_negatives(M.nu, M.ni, n, user.data(), pos.data(), m * C, seed, cand.data());
    pair_hard_negatives(M.nu, M.ni, n, user.data(), pos.data(), m, C, seed, M.k, M.wu.data(), M.wi.data(), M.bias.data(), neg.data(), score.data());
    EXPECT(neg.back() == 0xDEADu && score.back() == -77.0f);
    std::vector<unsigned> again((size_t)N);
    pair_hard_negatives(M.nu, M.ni, n, user.data(), pos.data(), m, C, seed, M.k, M.wu.data(), M.wi.data(), M.bias.data(), again.data(), nullptr);
    for (long q = 0; q < N; q++) {
        const float *urow = M.wu.data() + (size_t)user[(size_t)(q / m)] * (size_t)M.k;
        long best = -1;
        float bs = 0.0f;
        for (int i = 0; i < C; i++) {
            const unsigned c = cand[(size_t)q * (size_t)C + (size_t)i];
            const float s = pair_hard_score(M.k, urow, M.wi.data() + (size_t)c * (size_t)M.k, M.bias[c]);
            if (std::isnan(s)) continue;
            if (best < 0 || s > bs || (s == bs && (long)c < best)) { best = (long)c; bs = s; }
        }
        if (best < 0) {   // every candidate NaN: cand(q, 0)
            EXPECT(neg[(size_t)q] == cand[(size_t)q * (size_t)C] && std::isnan(score[(size_t)q]));
        } else {
            EXPECT((long)neg[(size_t)q] == best && score[(size_t)q] == bs && !std::isnan(score[(size_t)q]));
        }
        EXPECT(again[(size_t)q] == neg[(size_t)q]);
    }
}

static Model random_model(long nu, long ni, int k, unsigned seed) {
    Model M{nu, ni, k, {}, {}, {}};
    std::mt19937 rng(seed);
    std::normal_distribution<float> g(0.0f, 1.0f);
    M.wu.resize((size_t)nu * (size_t)k); M.wi.resize((size_t)ni * (size_t)k); M.bias.resize((size_t)ni);
    for (float &x : M.wu) x = g(rng);
    for (float &x : M.wi) x = g(rng);
    for (float &x : M.bias) x = 0.1f * g(rng);
    return M;
}

static void random_rows(long nu, long ni, long n, unsigned seed, std::vector<unsigned> &user, std::vector<unsigned> &pos) {
    std::mt19937 rng(seed);
    user.clear(); pos.clear();
    for (long r = 0; r < n; r++) {
        if (r > 10 && rng() % 6 == 0) { const size_t j = rng() % user.size(); user.push_back(user[j]); pos.push_back(pos[j]); continue; }
        user.push_back(3 + (unsigned)(rng() % (nu - 3)));
        pos.push_back((unsigned)(rng() % ni));
    }
    user[0] = 2;   // one row; users 0 and 1 have none
}

static int dump() {
    using namespace svdf;
    long nu, ni, n;
    int m, C, k;
    unsigned long long seed;
    if (std::scanf("%ld %ld %ld %d %d %llu %d", &nu, &ni, &n, &m, &C, &seed, &k) != 7) return 2;
    if (nu < 1 || ni < 1 || k < 1 || k > 1024 || nu > 100000 || ni > 100000) return 2;
    std::vector<unsigned> user((size_t)std::max<long>(n, 0)), pos(user.size());
    for (long r = 0; r < n; r++)
        if (std::scanf("%u %u", &user[(size_t)r], &pos[(size_t)r]) != 2) return 2;
    std::vector<float> wu((size_t)nu * (size_t)k), wi((size_t)ni * (size_t)k), bias((size_t)ni);
    for (std::vector<float> *v : {&wu, &wi, &bias})
        for (float &x : *v) {
            unsigned b;
            if (std::scanf("%x", &b) != 1) return 2;
            std::memcpy(&x, &b, 4);
        }
    try {
        pair_hard_check_pass(n, m, C);   // (before the columns are sized)
        std::vector<unsigned> neg((size_t)n * (size_t)m);
        std::vector<float> score(neg.size());
        pair_hard_negatives(nu, ni, n, user.data(), pos.data(), m, C, (uint64_t)seed, k, wu.data(), wi.data(), bias.data(), neg.data(), score.data());
        std::printf("neg");
        for (unsigned x : neg) std::printf(" %u", x);
        std::printf("\nscore");
        for (float x : score) std::printf(" %08x", bits(x));
        std::printf("\n");
    } catch (const std::runtime_error &e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}

int main(int argc, char **argv) {
    using namespace svdf;
    if (argc > 1 && std::string(argv[1]) == "dump") return dump();
    // ---- the pinned vectors (include/svdfeature_amd.h): m = 1, C = 2 has the candidates of the plain pass with num_neg 2
    {
        const unsigned user[3] = {4, 4, 9}, pos[3] = {10, 700, 10};
        Model M{10, 1200, 4, std::vector<float>(40, 0.0f), std::vector<float>(4800, 0.0f), std::vector<float>(1200)};
        unsigned neg[3];
        float score[3];
        for (unsigned c = 0; c < 1200; c++) M.bias[c] = (float)c;
        pair_hard_negatives(10, 1200, 3, user, pos, 1, 2, 12345, 4, M.wu.data(), M.wi.data(), M.bias.data(), neg, score);
        EXPECT(neg[0] == 607 && neg[1] == 1010 && neg[2] == 448 && score[0] == 607.0f && score[1] == 1010.0f && score[2] == 448.0f);
        for (unsigned c = 0; c < 1200; c++) M.bias[c] = -(float)c;
        pair_hard_negatives(10, 1200, 3, user, pos, 1, 2, 12345, 4, M.wu.data(), M.wi.data(), M.bias.data(), neg, score);
        EXPECT(neg[0] == 549 && neg[1] == 766 && neg[2] == 64 && score[2] == -64.0f);
    }
    // ---- the score: chains, pairing, tail; the key: order, -0, NaN
    {
        const float p[7] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f, 6.0f, 7.0f}, v[7] = {0.5f, 0.25f, 2.0f, 1.0f, 3.0f, 1.5f, 0.125f};
        EXPECT(pair_hard_score(7, p, v, 1.0f) == 1.0f + ((((0.5f + 6.0f) + (0.5f + 4.0f)) + 15.0f) + 9.0f + 0.875f));
        EXPECT(pair_hard_score(1, p, v, -0.0f) == 0.5f && bits(pair_hard_score(1, p, v, 0.0f)) == bits(0.5f));
        const float z = 0.0f;
        EXPECT(bits(pair_hard_score(1, &z, v, -0.0f)) == 0u);   // 0 + (-0 + 0 * x) is +0
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        EXPECT(pair_hard_key(nan, 5) == 0 && pair_hard_key(-inf, 0xFFFFFFFFu) > 0);
        EXPECT(pair_hard_key(0.0f, 9) == pair_hard_key(-0.0f, 9) && pair_hard_key(0.0f, 8) > pair_hard_key(-0.0f, 9));
        EXPECT(pair_hard_key(1.0f, 100) > pair_hard_key(0.5f, 1) && pair_hard_key(-1.0f, 1) < pair_hard_key(-0.5f, 100));
        EXPECT(pair_hard_key(inf, 7) > pair_hard_key(3e38f, 0) && pair_hard_key(-inf, 7) < pair_hard_key(-3e38f, 9));
        EXPECT(pair_hard_key(1e-45f, 3) > pair_hard_key(0.0f, 0) && pair_hard_key(-1e-45f, 0) < pair_hard_key(-0.0f, 3));
    }
    // ---- random sources and models against the definition: widths with tails 0 .. 3, num_cand below, at and above 64
    {
        std::vector<unsigned> user, pos, gu, gp;
        const long nu = 60, ni = 200, n = 400;
        random_rows(nu, ni, n, 31, user, pos);
        std::vector<size_t> at((size_t)n);
        for (size_t j = 0; j < at.size(); j++) at[j] = j;
        std::stable_sort(at.begin(), at.end(), [&](size_t a, size_t b) { return user[a] < user[b]; });
        for (size_t j : at) { gu.push_back(user[j]); gp.push_back(pos[j]); }
        const int shapes[9][2] = {{1, 1}, {1, 2}, {1, 7}, {2, 3}, {3, 5}, {4, 64}, {1, 65}, {1, 100}, {1, 256}};
        int w = 0;
        for (const auto &mc : shapes) {
            const int ks[7] = {1, 3, 4, 5, 7, 16, 66};
            const Model M = random_model(nu, ni, ks[w++ % 7], 100u + (unsigned)mc[1]);
            check_hard(M, user, pos, mc[0], mc[1], 99);
            check_hard(M, gu, gp, mc[0], mc[1], (uint64_t)1 << 63 | 5);
        }
        // ties: every item row and bias twice; all scores equal (+0 and -0 biases on a zero user matrix); NaN rows; +-inf biases
        Model T = random_model(nu, ni, 6, 7);
        for (long c = 0; c < ni / 2; c++) {
            std::copy(T.wi.begin() + c * 6, T.wi.begin() + c * 6 + 6, T.wi.begin() + (c + ni / 2) * 6);
            T.bias[(size_t)(c + ni / 2)] = T.bias[(size_t)c];
        }
        check_hard(T, user, pos, 1, 8, 3);
        Model Z = random_model(nu, ni, 5, 8);
        std::fill(Z.wu.begin(), Z.wu.end(), 0.0f);
        for (long c = 0; c < ni; c++) Z.bias[(size_t)c] = c % 2 ? 0.0f : -0.0f;
        check_hard(Z, user, pos, 2, 8, 4);
        Model Nn = random_model(nu, ni, 9, 9);
        for (long c = 0; c < ni; c += 3) Nn.wi[(size_t)c * 9 + (size_t)(c % 9)] = std::numeric_limits<float>::quiet_NaN();
        check_hard(Nn, user, pos, 1, 4, 5);
        std::fill(Nn.wu.begin() + 5 * 9, Nn.wu.begin() + 6 * 9, std::numeric_limits<float>::quiet_NaN());   // user 5: every score NaN
        Nn.wu[7 * 9 + 8] = std::numeric_limits<float>::quiet_NaN();                                         // user 7: one NaN in the tail
        check_hard(Nn, user, pos, 1, 4, 5);
        check_hard(Nn, user, pos, 1, 70, 5);
        Model I = random_model(nu, ni, 4, 10);
        for (long c = 0; c < ni; c += 5) I.bias[(size_t)c] = (c % 2 ? 1.0f : -1.0f) * std::numeric_limits<float>::infinity();
        check_hard(I, user, pos, 1, 8, 6);
    }
    // ---- C = 1 is the plain pass
    {
        std::vector<unsigned> user, pos;
        random_rows(60, 200, 300, 5, user, pos);
        const Model M = random_model(60, 200, 8, 3);
        std::vector<unsigned> a(900), b(900);
        pair_src_negatives(60, 200, 300, user.data(), pos.data(), 3, 11, a.data());
        pair_hard_negatives(60, 200, 300, user.data(), pos.data(), 3, 1, 11, 8, M.wu.data(), M.wi.data(), M.bias.data(), b.data(), nullptr);
        EXPECT(a == b);
    }
    // ---- the exhaustion of an entry's draws with a tiny bound: the message names the plain-rule pair index q * C + i
    {
        const long ni = 6400;
        std::vector<unsigned> user(6300, 0u), pos(6300);
        for (unsigned i = 0; i < 6300; i++) pos[i] = i;
        PairSrcLists L;
        pair_src_build(2, ni, 6300, user.data(), pos.data(), L);
        const Model M = random_model(2, ni, 3, 4);
        std::vector<unsigned> neg(6300), plain(6300 * 2);
        std::vector<float> score(6300);
        EXPECT(refused([&] { pair_hard_draw_host(L, ni, 6300, user.data(), 1, 2, 7, 3, M.wu.data(), M.wi.data(), M.bias.data(), neg.data(), score.data()); }).empty());
        for (unsigned v : neg) EXPECT(v >= 6300 && v < 6400);
        const std::string hard = refused([&] { pair_hard_draw_host(L, ni, 6300, user.data(), 1, 2, 7, 3, M.wu.data(), M.wi.data(), M.bias.data(), neg.data(), nullptr, 8); });
        const std::string same = refused([&] { pair_src_draw_host(L, ni, 6300, user.data(), 2, 7, plain.data(), 8); });
        EXPECT(hard.rfind("pair_source: pair ", 0) == 0 && hard.find(" found no negative in 8 draws") != std::string::npos && hard == same);
    }
    // ---- refusals
    {
        const unsigned user[3] = {1, 2, 9}, pos[3] = {5, 6, 7};
        const Model M = random_model(10, 30, 4, 2);
        unsigned out[6];
        auto pass = [&](long n, int m, int C) { return refused([&] { pair_hard_check_pass(n, m, C); }); };
        EXPECT(pass(3, 1, 1).empty() && pass(3, 256, 1).empty() && pass(3, 1, 256).empty() && pass(3, 16, 16).empty() && pass(3, 4, 64).empty());
        EXPECT(pass(3, 0, 2) == "pair_source: num_neg must be between 1 and 256" && pass(3, 257, 1) == "pair_source: num_neg must be between 1 and 256");
        EXPECT(pass(3, 1, 0) == "pair_source: num_cand must be between 1 and 256" && pass(3, 1, 257) == "pair_source: num_cand must be between 1 and 256");
        EXPECT(pass(3, 1, -1) == "pair_source: num_cand must be between 1 and 256");
        EXPECT(pass(3, 2, 129) == "pair_source: num_neg * num_cand must be at most 256" && pass(3, 256, 256) == "pair_source: num_neg * num_cand must be at most 256");
        EXPECT(pass(((1L << 31) - 16) / 8, 2, 4) == "pair_source: n * num_neg * num_cand must stay below 2^31 - 16");
        EXPECT(pass(((1L << 31) - 16) / 8 - 1, 2, 4).empty());
        auto call = [&](int k, const float *wu, unsigned *neg) {
            return refused([&] { pair_hard_negatives(10, 30, 3, user, pos, 2, 1, 1, k, wu, M.wi.data(), M.bias.data(), neg, nullptr); });
        };
        EXPECT(call(4, M.wu.data(), out).empty());
        EXPECT(call(0, M.wu.data(), out) == "pair_source: hard negatives need num_factor between 1 and 1024");
        EXPECT(call(1025, M.wu.data(), out) == "pair_source: hard negatives need num_factor between 1 and 1024");
        EXPECT(call(4, nullptr, out) == "pair_source: bad arguments" && call(4, M.wu.data(), nullptr) == "pair_source: bad arguments");
        const unsigned ubad[3] = {1, 10, 9};
        EXPECT(refused([&] { pair_hard_negatives(10, 30, 3, ubad, pos, 1, 2, 1, 4, M.wu.data(), M.wi.data(), M.bias.data(), out, nullptr); }) ==
               "user feature index exceed bound");
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

// check_ranklines_lists.cpp -- the host-only part of the USER lines of svdf_rank_eval*_lines / svdf_rank_topn_lines
// (svdfeature_amd/csrc/svdf_ranklines_lists.h: validation, the check of a side table's child ids, the cut of a piece at the entry budget,
// the words a piece uploads) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_ranklines_lists.cpp -o tools/check_ranklines_lists && tools/check_ranklines_lists
// Ragged, empty and long lines with repeated ids and any float value, every refusal, pieces under small and large budgets, and the packed
// words of every piece.  Exit status 0 and "ok" when all holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>

#include "svdf_ranklines_lists.h"

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

static svdf::RankLines lines_of(const int64_t *ptr, const unsigned *index, const float *value) {
    svdf::RankLines U;
    U.ptr = ptr; U.index = index; U.value = value;
    return U;
}

int main() {
    using namespace svdf;
    const long nu = 200;
    std::mt19937 rng(13);
    // ---- random ragged lines: 0 - 6 entries with repeated ids, an empty line, one line of 300 entries, values of every kind
    const long S = 150;
    std::vector<unsigned> idx;
    std::vector<float> val;
    std::vector<int64_t> ptr((size_t)S + 1, 0);
    for (long s = 0; s < S; s++) {
        long n = (long)(rng() % 7);
        if (s == 5) n = 0;
        if (s == 40) n = 300;
        for (long j = 0; j < n; j++) {
            const unsigned u = (unsigned)(rng() % nu);
            idx.push_back(u);
            val.push_back((float)((int)(rng() % 2001) - 1000) / 700.0f);
            if (rng() % 5 == 0) { idx.push_back(u); val.push_back(-0.0f); }   // a repeated id
        }
        ptr[(size_t)s + 1] = (int64_t)idx.size();
    }
    val[3] = std::numeric_limits<float>::quiet_NaN();   // any float value is legal
    val[4] = std::numeric_limits<float>::infinity();
    val[6] = 1.0f + 5e-7f;
    const RankLines U = lines_of(ptr.data(), idx.data(), val.data());
    EXPECT(refused([&] { rank_lines_validate("rank_eval", S, U, nu); }).empty());
    EXPECT(refused([&] { rank_lines_validate("rank_topn", S - 7, lines_of(ptr.data() + 7, idx.data(), val.data()), nu); }).empty());   // lines that start past entry 0
    // ---- pieces: whole sections, in order, all of them, within the budget unless one section alone exceeds it; the packed words are the lines
    for (int64_t budget : {(int64_t)1, (int64_t)7, (int64_t)100, (int64_t)299, (int64_t)300, (int64_t)100000, (int64_t)1 << 40}) {
        long s0 = 0, pieces = 0;
        while (s0 < S) {
            const long cap = std::min(S, s0 + 64);   // the caller's own cut
            const long s1 = rank_lines_piece("rank_topn", s0, cap, ptr.data(), budget);
            EXPECT(s1 > s0 && s1 <= cap);
            EXPECT(s1 == s0 + 1 || ptr[(size_t)s1] - ptr[(size_t)s0] <= budget);
            EXPECT(s1 == cap || ptr[(size_t)s1 + 1] - ptr[(size_t)s0] > budget);   // ... and no shorter than it must be
            std::vector<int> words(rank_lines_words(s0, s1, ptr.data()));
            rank_lines_pack(s0, s1, U, words.data());
            const size_t nsec = (size_t)(s1 - s0), n = (size_t)(ptr[(size_t)s1] - ptr[(size_t)s0]);
            EXPECT(words.size() == nsec + 1 + 2 * n && words[0] == 0 && words[nsec] == (int)n);
            for (long s = s0; s < s1; s++)
                for (int64_t j = ptr[(size_t)s]; j < ptr[(size_t)s + 1]; j++) {
                    const size_t q = (size_t)(j - ptr[(size_t)s0]);
                    EXPECT(q >= (size_t)words[(size_t)(s - s0)] && q < (size_t)words[(size_t)(s - s0) + 1]);
                    EXPECT((unsigned)words[nsec + 1 + q] == idx[(size_t)j]);
                    EXPECT(std::memcmp(&words[nsec + 1 + n + q], &val[(size_t)j], 4) == 0);   // the value's bits, NaN and -0 included
                }
            s0 = s1;
            pieces++;
        }
        EXPECT(s0 == S && pieces >= (S + 63) / 64);
        if (budget == 1) EXPECT(pieces > S / 2);   // only lines of no or one entry share a piece
    }
    // ---- no sections, all lines empty without arrays
    {
        const int64_t zeros[3] = {0, 0, 0};
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 0, RankLines(), nu); }).empty());
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(zeros, nullptr, nullptr), nu); }).empty());
        EXPECT(rank_lines_piece("rank_eval", 0, 2, zeros, 1) == 2 && rank_lines_words(0, 2, zeros) == 3);
        int words[3] = {-1, -1, -1};
        rank_lines_pack(0, 2, lines_of(zeros, nullptr, nullptr), words);
        EXPECT(words[0] == 0 && words[1] == 0 && words[2] == 0);
    }
    // ---- refusals
    {
        const unsigned u2[2] = {3, 199}, ubad[2] = {3, 200}, uhuge[2] = {4000000000u, 3};
        const float v2[2] = {0.5f, -2.0f};
        const int64_t p[3] = {0, 1, 2}, pdec[3] = {0, 2, 1}, pneg[3] = {-1, 1, 2};
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(p, u2, v2), nu); }).empty());
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(p, ubad, v2), nu); }) == "user feature index exceed bound");
        EXPECT(refused([&] { rank_lines_validate("rank_topn", 2, lines_of(p, uhuge, v2), nu); }) == "user feature index exceed bound");
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(pdec, u2, v2), nu); }) == "rank_eval: ul_ptr must not decrease");
        EXPECT(refused([&] { rank_lines_validate("rank_topn", 2, lines_of(pneg, u2, v2), nu); }) == "rank_topn: ul_ptr must start at >= 0");
        EXPECT(refused([&] { rank_lines_validate("rank_topn", 2, lines_of(p, nullptr, v2), nu); }) == "rank_topn: ul_index / ul_value is missing");
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(p, u2, nullptr), nu); }) == "rank_eval: ul_index / ul_value is missing");
        EXPECT(refused([&] { rank_lines_validate("rank_eval", 2, lines_of(nullptr, u2, v2), nu); }) == "rank_eval: ul_ptr is missing");
        const int64_t big[2] = {0, (int64_t)1 << 30};
        EXPECT(refused([&] { rank_lines_piece("rank_topn", 0, 1, big, 100); }) == "rank_topn: one section with more than 2^30 line entries");
        // a side table's child ids against their id space; an empty table
        const std::vector<unsigned> kids = {0, 199, 7, 7}, out = {0, 200};
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", kids, nu); }).empty());
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", std::vector<unsigned>(), nu); }).empty());
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", out, nu); }) == "rank_eval: feature_user: child index exceed bound");
        EXPECT(refused([&] { rank_lines_check_children("rank_topn", "feature_item", kids, 199); }) == "rank_topn: feature_item: child index exceed bound");
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

// check_rankcand_lists.cpp -- the host-only part of the candidate lists of svdf_rank_eval*_cand / svdf_rank_topn_cand
// (svdfeature_amd/csrc/svdf_rankcand_lists.h: validation, a section's ranked set, the index of every positive in it, the cut of a piece at
// the entry budget, the tile table) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_rankcand_lists.cpp -o tools/check_rankcand_lists && tools/check_rankcand_lists
// Hand-made and random lists: duplicates, empty lists, positives listed and not listed, a list that covers the catalogue, every refusal,
// pieces under small and large budgets with one section larger than the budget, tiles that never cross a section.  Exit status 0 and "ok"
// when all holds.  With the argument "dump" it reads `S num_item positions`, then per section its candidates and (positions) its positives as
// `n id ..` lines from standard input and prints the ranked sets, the positives' indices and the tile table of one piece: the form
// tests/test_rank_cand.py compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>

#include "svdf_rankcand_lists.h"

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

struct Lists {
    std::vector<int64_t> cand_ptr{0}, pos_ptr{0};
    std::vector<unsigned> cand, pos;
};

// the ranked sets, indices and sizes against std::set; the tiles and pieces against their definitions
static void check_lists(const Lists &in, long S, long ni, bool positions) {
    using namespace svdf;
    RankCandLists L;
    EXPECT(refused([&] { rank_cand_validate("rank_eval", S, in.cand_ptr.data(), in.cand.data(), ni); }).empty());
    rank_cand_build(S, in.cand_ptr.data(), in.cand.data(), positions ? in.pos_ptr.data() : nullptr, in.pos.data(), ni, L);
    EXPECT((long)L.ranked.size() == S && (long)L.first.size() == S + 1 && L.first[0] == 0);
    EXPECT(L.pos_at.size() == (positions ? in.pos.size() : 0));
    for (long s = 0; s < S; s++) {
        std::set<unsigned> want(in.cand.begin() + in.cand_ptr[(size_t)s], in.cand.begin() + in.cand_ptr[(size_t)s + 1]);
        const bool has_pos = positions && in.pos_ptr[(size_t)s + 1] > in.pos_ptr[(size_t)s];
        if (positions) want.insert(in.pos.begin() + in.pos_ptr[(size_t)s], in.pos.begin() + in.pos_ptr[(size_t)s + 1]);
        EXPECT(L.ranked[(size_t)s] == (int)want.size());
        const int64_t a = L.first[(size_t)s], b = L.first[(size_t)s + 1];
        if (positions && !has_pos) { EXPECT(a == b); continue; }   // not kept: nothing of it is scored
        EXPECT(b - a == (int64_t)want.size());
        int64_t q = a;
        for (unsigned c : want) { EXPECT(L.ids[(size_t)q] == (int)c); q++; }   // distinct, ascending
        if (positions)
            for (int64_t j = in.pos_ptr[(size_t)s]; j < in.pos_ptr[(size_t)s + 1]; j++) {
                const int64_t at = L.pos_at[(size_t)j];
                EXPECT(at >= a && at < b && L.ids[(size_t)at] == (int)in.pos[(size_t)j]);
            }
    }
    for (int threads : {2, 3, 16, 1000}) {   // ranges of sections built side by side: the same lists
        RankCandLists M;
        rank_cand_build(S, in.cand_ptr.data(), in.cand.data(), positions ? in.pos_ptr.data() : nullptr, in.pos.data(), ni, M, threads);
        EXPECT(M.ranked == L.ranked && M.first == L.first && M.ids == L.ids && M.pos_at == L.pos_at);
    }
    const int64_t *extra[2] = {positions ? in.pos_ptr.data() : nullptr, nullptr};
    for (int64_t budget : {(int64_t)1, (int64_t)50, (int64_t)257, (int64_t)1000, (int64_t)1 << 40}) {
        long s0 = 0, pieces = 0;
        std::vector<int> tq0, tsec;
        while (s0 < S) {
            const long s1 = rank_cand_piece("rank_eval", s0, S, L.first, extra, 2, budget);
            EXPECT(s1 > s0 && s1 <= S);
            auto load = [&](long e) { return (L.first[(size_t)e] - L.first[(size_t)s0]) + (e - s0) + (positions ? in.pos_ptr[(size_t)e] - in.pos_ptr[(size_t)s0] : 0); };
            EXPECT(s1 == s0 + 1 || load(s1) <= budget);   // whole sections within the budget; a larger section is a piece of its own
            EXPECT(s1 == S || load(s1 + 1) > budget);     // ... and no shorter than it must be
            rank_cand_tiles(s0, s1, L.first, tq0, tsec);
            EXPECT(tq0.size() == tsec.size() + 1 && tq0[0] == 0 && tq0.back() == (int)(L.first[(size_t)s1] - L.first[(size_t)s0]));
            for (size_t t = 0; t < tsec.size(); t++) {
                const int n = tq0[t + 1] - tq0[t];
                const int64_t a = L.first[(size_t)(s0 + tsec[t])] - L.first[(size_t)s0], b = L.first[(size_t)(s0 + tsec[t]) + 1] - L.first[(size_t)s0];
                EXPECT(n >= 1 && n <= RANK_CAND_TILE);
                EXPECT(tq0[t] >= a && tq0[t + 1] <= b);   // never crosses a section
                EXPECT(n == RANK_CAND_TILE || tq0[t + 1] == b);   // only a section's last tile is short
                EXPECT(t == 0 || tsec[t] >= tsec[t - 1]);
            }
            s0 = s1;
            pieces++;
        }
        EXPECT(s0 == S);
        if (budget == 1) EXPECT(pieces == S);
        if (budget == (int64_t)1 << 40) EXPECT(pieces == (S > 0 ? 1 : 0));
    }
}

static int dump() {
    using namespace svdf;
    long S, ni;
    int positions;
    if (std::scanf("%ld %ld %d", &S, &ni, &positions) != 3) return 2;
    Lists in;
    for (long s = 0; s < S; s++)
        for (int part = 0; part < 1 + positions; part++) {
            long n;
            if (std::scanf("%ld", &n) != 1) return 2;
            for (long j = 0; j < n; j++) {
                unsigned v;
                if (std::scanf("%u", &v) != 1) return 2;
                (part ? in.pos : in.cand).push_back(v);
            }
            if (part) in.pos_ptr.push_back((int64_t)in.pos.size()); else in.cand_ptr.push_back((int64_t)in.cand.size());
        }
    try {
        RankCandLists L;
        rank_cand_validate("rank_eval", S, in.cand_ptr.data(), in.cand.data(), ni);
        rank_cand_build(S, in.cand_ptr.data(), in.cand.data(), positions ? in.pos_ptr.data() : nullptr, in.pos.data(), ni, L);
        std::vector<int> tq0, tsec;
        rank_cand_tiles(0, S, L.first, tq0, tsec);
        auto line = [](const char *name, auto &v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); };
        line("ranked", L.ranked); line("first", L.first); line("ids", L.ids); line("pos_at", L.pos_at); line("tile_q0", tq0); line("tile_sec", tsec);
    } catch (const std::runtime_error &e) {
        std::printf("refused %s\n", e.what());
    }
    return 0;
}

int main(int argc, char **argv) {
    using namespace svdf;
    if (argc > 1 && std::string(argv[1]) == "dump") return dump();
    // ---- a hand-made case: duplicates, an empty list, a positive listed and one not listed, a section without positives
    {
        Lists in;
        in.cand = {5, 3, 5, 9, 3, /* s1: none */ /* s2 */ 7, 7, 7, /* s3 */ 1, 2};
        in.cand_ptr = {0, 5, 5, 8, 10};
        in.pos = {9, 4, /* s1 */ 6, 2, /* s2: none */ /* s3 */ 0};
        in.pos_ptr = {0, 2, 4, 4, 5};
        RankCandLists L;
        rank_cand_build(4, in.cand_ptr.data(), in.cand.data(), in.pos_ptr.data(), in.pos.data(), 10, L);
        EXPECT((L.ranked == std::vector<int>{4, 2, 1, 3}));                       // {3 4 5 9} {2 6} {7} {0 1 2}
        EXPECT((L.ids == std::vector<int>{3, 4, 5, 9, 2, 6, 0, 1, 2}));           // section 2 has no positive: not kept
        EXPECT((L.first == std::vector<int64_t>{0, 4, 6, 6, 9}));
        EXPECT((L.pos_at == std::vector<int64_t>{3, 1, 5, 4, 6}));
        rank_cand_build(4, in.cand_ptr.data(), in.cand.data(), nullptr, nullptr, 10, L);   // top-N: the lists alone, every section kept
        EXPECT((L.ranked == std::vector<int>{3, 0, 1, 2}) && (L.ids == std::vector<int>{3, 5, 9, 7, 1, 2}) && L.pos_at.empty());
        check_lists(in, 4, 10, true);
        check_lists(in, 4, 10, false);
    }
    // ---- random lists: lengths 0, 1, 63, 64, 65, 129, 257 and the whole catalogue; duplicates; positives inside and outside the list
    {
        const long ni = 1200, S = 60;
        std::mt19937 rng(17);
        const long lens[8] = {0, 1, 63, 64, 65, 129, 257, ni};
        Lists in;
        for (long s = 0; s < S; s++) {
            const long n = s < 8 ? lens[s] : (long)(rng() % 300);
            if (n == ni) for (long j = 0; j < ni; j++) in.cand.push_back((unsigned)((j * 7) % ni));   // a permutation of the catalogue
            else for (long j = 0; j < n; j++) in.cand.push_back((unsigned)(rng() % ni));
            const size_t a = (size_t)in.cand_ptr.back();
            if (n > 4 && s % 3 == 0) { in.cand.push_back(in.cand[a]); in.cand.push_back(in.cand[a + 2]); }   // repeated ids
            in.cand_ptr.push_back((int64_t)in.cand.size());
            std::set<unsigned> pos;
            const long npos = s == 9 ? 0 : 1 + (long)(rng() % 4);
            while ((long)pos.size() < npos) pos.insert(n > 0 && rng() % 2 ? in.cand[a + rng() % (size_t)n] : (unsigned)(rng() % ni));
            in.pos.insert(in.pos.end(), pos.begin(), pos.end());
            in.pos_ptr.push_back((int64_t)in.pos.size());
        }
        check_lists(in, S, ni, true);
        check_lists(in, S, ni, false);
        // lists that start past entry 0
        Lists cut;
        cut.cand = in.cand; cut.pos = in.pos;
        cut.cand_ptr.assign(in.cand_ptr.begin() + 5, in.cand_ptr.end());
        cut.pos_ptr.assign(in.pos_ptr.begin() + 5, in.pos_ptr.end());
        RankCandLists A, B;
        rank_cand_build(S - 5, cut.cand_ptr.data(), cut.cand.data(), cut.pos_ptr.data(), cut.pos.data(), ni, A);
        rank_cand_build(S, in.cand_ptr.data(), in.cand.data(), in.pos_ptr.data(), in.pos.data(), ni, B);
        EXPECT(A.ids.size() == B.ids.size() - (size_t)B.first[5] && A.pos_at.size() == B.pos_at.size() - (size_t)in.pos_ptr[5]);
        for (size_t j = 0; j < A.pos_at.size(); j++) EXPECT(A.pos_at[j] == B.pos_at[j + (size_t)in.pos_ptr[5]] - B.first[5]);
    }
    // ---- no sections; all lists empty without arrays
    {
        const int64_t zeros[3] = {0, 0, 0};
        RankCandLists L;
        EXPECT(refused([&] { rank_cand_validate("rank_eval", 0, nullptr, nullptr, 10); }).empty());
        EXPECT(refused([&] { rank_cand_validate("rank_topn", 2, zeros, nullptr, 10); }).empty());
        rank_cand_build(2, zeros, nullptr, nullptr, nullptr, 10, L);
        EXPECT((L.ranked == std::vector<int>{0, 0}) && L.ids.empty());
        rank_cand_build(0, nullptr, nullptr, nullptr, nullptr, 10, L);
        EXPECT(L.ranked.empty() && L.first.size() == 1);
        std::vector<int> tq0, tsec;
        rank_cand_tiles(0, 2, std::vector<int64_t>{0, 0, 0}, tq0, tsec);
        EXPECT(tq0.size() == 1 && tq0[0] == 0 && tsec.empty());
    }
    // ---- refusals
    {
        const unsigned c2[2] = {3, 9}, cbad[2] = {3, 10}, chuge[2] = {4000000000u, 3};
        const int64_t p[3] = {0, 1, 2}, pdec[3] = {0, 2, 1}, pneg[3] = {-1, 1, 2};
        EXPECT(refused([&] { rank_cand_validate("rank_eval", 2, p, c2, 10); }).empty());
        EXPECT(refused([&] { rank_cand_validate("rank_eval", 2, p, cbad, 10); }) == "sample item index exceed bound");
        EXPECT(refused([&] { rank_cand_validate("rank_topn", 2, p, chuge, 10); }) == "sample item index exceed bound");
        EXPECT(refused([&] { rank_cand_validate("rank_eval", 2, pdec, c2, 10); }) == "rank_eval: cand_ptr must not decrease");
        EXPECT(refused([&] { rank_cand_validate("rank_topn", 2, pneg, c2, 10); }) == "rank_topn: cand_ptr must start at >= 0");
        EXPECT(refused([&] { rank_cand_validate("rank_topn", 2, p, nullptr, 10); }) == "rank_topn: cand_item is missing");
        EXPECT(refused([&] { rank_cand_validate("rank_eval", 2, nullptr, c2, 10); }) == "rank_eval: cand_ptr is missing");
        RankCandLists L;
        const unsigned prep[2] = {4, 4}, pbad[2] = {4, 10};
        const int64_t pp[3] = {0, 0, 2};
        EXPECT(refused([&] { rank_cand_build(2, p, c2, pp, prep, 10, L); }) == "rank_eval: a positive item is repeated inside a section");
        EXPECT(refused([&] { rank_cand_build(2, p, c2, pp, pbad, 10, L); }) == "sample item index exceed bound");
        EXPECT(refused([&] { rank_cand_build(2, p, c2, p, prep, 10, L); }).empty());   // the same id in two sections is no repeat
        const unsigned p3[3] = {4, 10, 10};
        const int64_t c3[4] = {0, 1, 2, 2}, pp3[4] = {0, 1, 1, 3};                     // section 0 out of bound?  no: section 2 is, and repeats; bound is checked first
        for (int threads : {1, 2, 3})
            EXPECT(refused([&] { rank_cand_build(3, c3, c2, pp3, p3, 10, L, threads); }) == "sample item index exceed bound");
        const unsigned p4[4] = {4, 4, 10, 3};
        const int64_t pp4[4] = {0, 2, 3, 4};                                           // section 0 repeats a positive, section 1 is out of bound: the first section's refusal
        for (int threads : {1, 2, 3})
            EXPECT(refused([&] { rank_cand_build(3, c3, c2, pp4, p4, 10, L, threads); }) == "rank_eval: a positive item is repeated inside a section");
        const std::vector<int64_t> big = {0, (int64_t)1 << 29};
        EXPECT(refused([&] { rank_cand_piece("rank_topn", 0, 1, big, nullptr, 0, 100); }) == "rank_topn: one section with more than 2^29 candidates");
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

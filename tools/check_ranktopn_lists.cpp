// check_ranktopn_lists.cpp -- the host-only part of svdf_rank_topn (svdfeature_amd/csrc/svdf_ranktopn_lists.h: list validation and the cut
// into pieces) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_ranktopn_lists.cpp -o tools/check_ranktopn_lists && tools/check_ranktopn_lists
// Ragged, duplicate and empty ban lists, every refusal, and pieces under small and large workspaces.  Exit status 0 and "ok" when all holds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>

#include "svdf_ranktopn_lists.h"

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

int main() {
    using namespace svdf;
    const long nu = 50, ni = 517;
    std::mt19937 rng(7);
    // ---- random ragged lists: 0 - 40 bans with duplicates, an empty list, a list that bans all but 5 items, a user in three sections
    const long S = 203;
    std::vector<unsigned> user((size_t)S), ban;
    std::vector<int64_t> ptr((size_t)S + 1, 0);
    std::vector<std::set<unsigned>> want((size_t)S);
    for (long s = 0; s < S; s++) {
        user[(size_t)s] = (s == 0 || s == 50 || s == 101) ? 7u : (unsigned)(rng() % nu);
        long n = (long)(rng() % 41);
        if (s == 20) n = 0;
        if (s == 30) { for (unsigned b = 5; b < (unsigned)ni; b++) { ban.push_back(b); want[(size_t)s].insert(b); } n = 3; }   // ... and three duplicates
        for (long j = 0; j < n; j++) {
            const unsigned b = (s == 30) ? 5u + (unsigned)(rng() % (ni - 5)) : (unsigned)(rng() % ni);
            ban.push_back(b);
            want[(size_t)s].insert(b);
            if (rng() % 4 == 0) ban.push_back(b);   // a duplicate entry
        }
        ptr[(size_t)s + 1] = (int64_t)ban.size();
    }
    for (int top_n : {1, 10, 256}) {
        RankTopnLists L;
        rank_topn_validate(S, user.data(), ptr.data(), ban.data(), nu, ni, top_n, L);
        EXPECT(L.ban_first.size() == (size_t)S + 1 && L.count.size() == (size_t)S);
        for (long s = 0; s < S; s++) {
            const std::vector<int> got(L.ban_ids.begin() + L.ban_first[(size_t)s], L.ban_ids.begin() + L.ban_first[(size_t)s + 1]);
            const std::vector<int> exp(want[(size_t)s].begin(), want[(size_t)s].end());   // a set iterates ascending
            EXPECT(got == exp);
            EXPECT(L.count[(size_t)s] == (int)std::min<long>(top_n, ni - (long)exp.size()));
        }
        EXPECT(L.count[30] == std::min(top_n, 5) && L.ban_first[21] == L.ban_first[20]);
        // ---- pieces: whole sections, in order, all of them, never more than the workspace holds
        for (long max_lists : {1L, 5L, 64L, 100L, 130L, 1000L}) {
            long s0 = 0, pieces = 0;
            while (s0 < S) {
                const long s1 = rank_topn_piece(s0, S, max_lists, L.ban_first);
                EXPECT(s1 > s0 && s1 <= S && s1 - s0 <= max_lists);
                EXPECT(s1 == S || max_lists <= 64 || (s1 - s0) % 64 == 0);
                s0 = s1;
                pieces++;
            }
            EXPECT(s0 == S && pieces >= (S + max_lists - 1) / max_lists);
        }
    }
    // ---- ban_ptr == NULL, no sections, empty ban array
    {
        RankTopnLists L;
        rank_topn_validate(S, user.data(), nullptr, nullptr, nu, ni, 300, L);
        EXPECT(L.ban_ids.empty() && L.count[0] == 300 && L.ban_first[(size_t)S] == 0);
        rank_topn_validate(0, nullptr, nullptr, nullptr, nu, ni, 10, L);
        EXPECT(L.ban_first.size() == 1 && L.count.empty());
        const int64_t zeros[3] = {0, 0, 0};
        rank_topn_validate(2, user.data(), zeros, nullptr, nu, ni, 10, L);
        EXPECT(L.count[1] == 10);
        EXPECT(rank_topn_piece(0, 1, 1000, L.ban_first) == 1);
    }
    // ---- refusals
    {
        RankTopnLists L;
        const unsigned u2[2] = {1, 2}, ubad[2] = {1, 50}, b2[2] = {3, 4}, bbad[2] = {3, 517}, bhuge[2] = {3, 4000000000u};
        const int64_t p[3] = {0, 1, 2}, pdec[3] = {0, 2, 1}, pneg[3] = {-1, 1, 2};
        EXPECT(refused([&] { rank_topn_validate(2, ubad, p, b2, nu, ni, 5, L); }) == "user feature index exceed bound");
        EXPECT(refused([&] { rank_topn_validate(2, u2, p, bbad, nu, ni, 5, L); }) == "sample item index exceed bound");
        EXPECT(refused([&] { rank_topn_validate(2, u2, p, bhuge, nu, ni, 5, L); }) == "sample item index exceed bound");
        EXPECT(refused([&] { rank_topn_validate(2, u2, pdec, b2, nu, ni, 5, L); }) == "rank_topn: ban_ptr must not decrease");
        EXPECT(refused([&] { rank_topn_validate(2, u2, pneg, b2, nu, ni, 5, L); }) == "rank_topn: ban_ptr must start at >= 0");
        EXPECT(refused([&] { rank_topn_validate(2, u2, p, nullptr, nu, ni, 5, L); }) == "rank_topn: ban_item is missing");
        EXPECT(refused([&] { rank_topn_validate(2, nullptr, p, b2, nu, ni, 5, L); }) == "rank_topn: bad arguments");
        EXPECT(refused([&] { rank_topn_validate(-1, u2, p, b2, nu, ni, 5, L); }) == "rank_topn: bad arguments");
        EXPECT(refused([&] { rank_topn_validate(2, u2, p, b2, nu, ni, 5, L); }).empty());
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

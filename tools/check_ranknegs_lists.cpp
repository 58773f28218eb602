// check_ranknegs_lists.cpp -- the host-only part of svdf_rank_negatives / svdf_rank_eval*_sampled
// (svdfeature_amd/csrc/svdf_ranknegs_lists.h: the rule that draws a section's negatives, the validation of bans and positives, the
// excluded lists, the availability rule, the pair offsets that follow from sizes alone; with svdf_rankcand_lists.h the pieces and the tile
// table over them) as a stand-alone program, meant to be built with a sanitizer:
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_ranknegs_lists.cpp -o tools/check_ranknegs_lists && tools/check_ranknegs_lists
// The pinned vectors of the rule, hand-made and random sections (duplicated bans, sections without positives, a ban that is the first draw),
// every refusal, the availability rule at its edge, the arithmetic offsets and tiles.  Exit status 0 and "ok" when all holds.  With the
// argument "dump" it reads `S num_item num_neg seed`, then per section its bans and its positives as `n id ..` lines from standard input and
// prints the negatives, the excluded lists, the offsets and the tile table of one piece: the form tests/test_rank_negs.py compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <stdexcept>

#include "svdf_rankcand_lists.h"
#include "svdf_ranknegs_lists.h"

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
    std::vector<int64_t> ban_ptr{0}, pos_ptr{0};
    std::vector<unsigned> ban, pos;
};

// the negatives against the sequential definition over std::set; the excluded lists, offsets, pieces and tiles against their definitions
static void check_lists(const Lists &in, long S, long ni, int num_neg, uint64_t seed) {
    using namespace svdf;
    RankNegsLists L;
    EXPECT(refused([&] { rank_negs_build(S, in.pos_ptr.data(), in.pos.data(), in.ban_ptr.data(), in.ban.data(), ni, num_neg, L); }).empty());
    std::vector<int> neg((size_t)S * (size_t)num_neg + 1, -7);
    rank_negs_host(S, in.pos_ptr.data(), in.pos.data(), in.ban_ptr.data(), in.ban.data(), ni, num_neg, seed, neg.data());
    EXPECT(neg.back() == -7);
    EXPECT((long)L.ranked.size() == S && (long)L.first.size() == S + 1 && (long)L.ex_first.size() == S + 1 && L.first[0] == 0 && L.ex_first[0] == 0);
    for (long s = 0; s < S; s++) {
        const int64_t npos = in.pos_ptr[(size_t)s + 1] - in.pos_ptr[(size_t)s];
        const int *row = neg.data() + (size_t)s * (size_t)num_neg;
        if (npos == 0) {
            EXPECT(L.ranked[(size_t)s] == num_neg && L.first[(size_t)s + 1] == L.first[(size_t)s] && L.ex_first[(size_t)s + 1] == L.ex_first[(size_t)s]);
            for (int j = 0; j < num_neg; j++) EXPECT(row[j] == -1);
            continue;
        }
        std::set<unsigned> ex(in.ban.begin() + in.ban_ptr[(size_t)s], in.ban.begin() + in.ban_ptr[(size_t)s + 1]);
        ex.insert(in.pos.begin() + in.pos_ptr[(size_t)s], in.pos.begin() + in.pos_ptr[(size_t)s + 1]);
        EXPECT(L.ex_first[(size_t)s + 1] - L.ex_first[(size_t)s] == (int64_t)ex.size());
        int64_t q = L.ex_first[(size_t)s];
        for (unsigned c : ex) { EXPECT(L.ex_ids[(size_t)q] == (int)c); q++; }   // distinct, ascending
        EXPECT(L.ranked[(size_t)s] == (int)npos + num_neg && L.first[(size_t)s + 1] - L.first[(size_t)s] == npos + num_neg);
        const uint64_t stream = rank_negs_stream(seed, (uint64_t)s);
        std::set<unsigned> seen = ex;
        int have = 0;
        for (uint64_t t = 0; have < num_neg; t++) {
            const unsigned id = rank_negs_draw(stream, t, (unsigned)ni);
            EXPECT((long)id < ni);
            if (!seen.insert(id).second) continue;
            EXPECT(row[have] == (int)id);
            have++;
        }
    }
    for (int threads : {2, 3, 16, 1000}) {   // ranges of sections built side by side: the same lists
        RankNegsLists M;
        rank_negs_build(S, in.pos_ptr.data(), in.pos.data(), in.ban_ptr.data(), in.ban.data(), ni, num_neg, M, threads);
        EXPECT(M.ranked == L.ranked && M.first == L.first && M.ex_first == L.ex_first && M.ex_ids == L.ex_ids);
    }
    const int64_t *extra[2] = {in.pos_ptr.data(), L.ex_first.data()};
    for (int64_t budget : {(int64_t)1, (int64_t)300, (int64_t)5000, (int64_t)1 << 40}) {
        long s0 = 0, pieces = 0;
        std::vector<int> tq0, tsec;
        while (s0 < S) {
            const long s1 = rank_cand_piece("rank_eval", s0, S, L.first, extra, 2, budget);
            EXPECT(s1 > s0 && s1 <= S);
            auto load = [&](long e) {
                return (L.first[(size_t)e] - L.first[(size_t)s0]) + (e - s0) + (in.pos_ptr[(size_t)e] - in.pos_ptr[(size_t)s0]) +
                       (L.ex_first[(size_t)e] - L.ex_first[(size_t)s0]);
            };
            EXPECT(s1 == s0 + 1 || load(s1) <= budget);
            EXPECT(s1 == S || load(s1 + 1) > budget);
            rank_cand_tiles(s0, s1, L.first, tq0, tsec);
            EXPECT(tq0.size() == tsec.size() + 1 && tq0[0] == 0 && tq0.back() == (int)(L.first[(size_t)s1] - L.first[(size_t)s0]));
            for (size_t t = 0; t < tsec.size(); t++) {
                const int n = tq0[t + 1] - tq0[t];
                const int64_t a = L.first[(size_t)(s0 + tsec[t])] - L.first[(size_t)s0], b = L.first[(size_t)(s0 + tsec[t]) + 1] - L.first[(size_t)s0];
                EXPECT(n >= 1 && n <= RANK_CAND_TILE && tq0[t] >= a && tq0[t + 1] <= b);   // never crosses a section
                EXPECT(n == RANK_CAND_TILE || tq0[t + 1] == b);
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
    int num_neg;
    unsigned long long seed;
    if (std::scanf("%ld %ld %d %llu", &S, &ni, &num_neg, &seed) != 4) return 2;
    Lists in;
    for (long s = 0; s < S; s++)
        for (int part = 0; part < 2; part++) {
            long n;
            if (std::scanf("%ld", &n) != 1) return 2;
            for (long j = 0; j < n; j++) {
                unsigned v;
                if (std::scanf("%u", &v) != 1) return 2;
                (part ? in.pos : in.ban).push_back(v);
            }
            if (part) in.pos_ptr.push_back((int64_t)in.pos.size()); else in.ban_ptr.push_back((int64_t)in.ban.size());
        }
    try {
        RankNegsLists L;
        rank_negs_build(S, in.pos_ptr.data(), in.pos.data(), in.ban_ptr.data(), in.ban.data(), ni, num_neg, L);
        std::vector<int> neg((size_t)S * (size_t)num_neg);
        rank_negs_host(S, in.pos_ptr.data(), in.pos.data(), in.ban_ptr.data(), in.ban.data(), ni, num_neg, (uint64_t)seed, neg.data());
        std::vector<int> tq0, tsec;
        rank_cand_tiles(0, S, L.first, tq0, tsec);
        auto line = [](const char *name, auto &v) { std::printf("%s", name); for (auto x : v) std::printf(" %lld", (long long)x); std::printf("\n"); };
        line("neg", neg); line("ranked", L.ranked); line("ex_first", L.ex_first); line("ex_ids", L.ex_ids); line("first", L.first);
        line("tile_q0", tq0); line("tile_sec", tsec);
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
        EXPECT(rank_negs_stream(12345, 0) == 0x22118258a9d111a0ull && rank_negs_stream(12345, 7) == 0x6e7411b06820371cull);
        const unsigned d0[6] = {18, 601, 213, 846, 111, 362}, d7[8] = {1196, 25, 1196, 303, 504, 615, 588, 726};
        for (int t = 0; t < 6; t++) EXPECT(rank_negs_draw(rank_negs_stream(12345, 0), (uint64_t)t, 1200) == d0[t]);
        for (int t = 0; t < 8; t++) EXPECT(rank_negs_draw(rank_negs_stream(12345, 7), (uint64_t)t, 1200) == d7[t]);
        const int ex[2] = {25, 303};
        int neg[5];
        std::vector<uint64_t> mark((1200 + 63) / 64, 0);
        EXPECT(rank_negs_section(rank_negs_stream(12345, 7), 1200, ex, 2, 5, neg, mark) == 8);
        EXPECT(neg[0] == 1196 && neg[1] == 504 && neg[2] == 615 && neg[3] == 588 && neg[4] == 726);
        for (uint64_t w : mark) EXPECT(w == 0);
        // through the export's function: section 7 of eight, its positive 25 and its ban 303 (given twice); the others have no positive
        const int64_t pos_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 1}, ban_ptr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 2};
        const unsigned pos[1] = {25}, ban[2] = {303, 303};
        std::vector<int> out(8 * 5);
        rank_negs_host(8, pos_ptr, pos, ban_ptr, ban, 1200, 5, 12345, out.data());
        for (int j = 0; j < 35; j++) EXPECT(out[(size_t)j] == -1);
        for (int j = 0; j < 5; j++) EXPECT(out[35 + (size_t)j] == neg[j]);
        // the top of the range: the largest product of the map stays below 2^64, the largest id below num_item
        EXPECT((unsigned)((0xffffffffull * 0x7fffffffull) >> 32) == 0x7ffffffeu);
        EXPECT(rank_negs_table(1) == 2 && rank_negs_table(64) == 128 && rank_negs_table(65) == 256 && rank_negs_table(4096) == 8192);
    }
    // ---- random sections: 0 .. 190 bans with duplicates, 0 .. 3 positives, a ban that is the section's first draw
    for (int num_neg : {1, 63, 64, 65, 99, 500}) {
        const long ni = 1200, S = 60;
        std::mt19937 rng(17 + (unsigned)num_neg);
        Lists in;
        for (long s = 0; s < S; s++) {
            std::set<unsigned> pos;
            const long npos = s == 9 ? 0 : (long)(rng() % 4);
            while ((long)pos.size() < npos) pos.insert((unsigned)(rng() % ni));
            const long nban = (long)(rng() % 191);
            const size_t a = in.ban.size();
            for (long j = 0; j < nban; j++) {
                const unsigned b = j > 3 && rng() % 8 == 0 ? in.ban[a + rng() % (size_t)j] : (unsigned)(rng() % ni);
                if (!pos.count(b)) in.ban.push_back(b);
            }
            const unsigned d = rank_negs_draw(rank_negs_stream(99, (uint64_t)s), 0, (unsigned)ni);
            if (s % 5 == 0 && !pos.count(d)) in.ban.push_back(d);
            in.ban_ptr.push_back((int64_t)in.ban.size());
            in.pos.insert(in.pos.end(), pos.begin(), pos.end());
            in.pos_ptr.push_back((int64_t)in.pos.size());
        }
        check_lists(in, S, ni, num_neg, 99);
        // without bans at all
        std::vector<int> a((size_t)S * (size_t)num_neg), b(a.size());
        const std::vector<int64_t> zeros((size_t)S + 1, 0);
        rank_negs_host(S, in.pos_ptr.data(), in.pos.data(), nullptr, nullptr, ni, num_neg, 99, a.data());
        rank_negs_host(S, in.pos_ptr.data(), in.pos.data(), zeros.data(), nullptr, ni, num_neg, 99, b.data());
        EXPECT(a == b);
    }
    // ---- the availability rule at its edges, no sections, the largest table
    {
        RankNegsLists L;
        const int64_t p1[2] = {0, 1}, p0[2] = {0, 0};
        const unsigned pos[1] = {0};
        std::vector<unsigned> ban;
        for (unsigned b = 1; b < 1000; b++) ban.push_back(b);   // with the positive 1000 of 1200 excluded: 200 left
        const int64_t b999[2] = {0, 999};
        EXPECT(refused([&] { rank_negs_build(1, p1, pos, b999, ban.data(), 1200, 100, L); }).empty());
        EXPECT(L.ranked[0] == 101 && L.first[1] == 101 && L.ex_first[1] == 1000);
        EXPECT(refused([&] { rank_negs_build(1, p1, pos, b999, ban.data(), 1200, 101, L); }) ==
               "rank_eval: section 0 leaves 200 items to draw 101 negatives from 1200; list its candidates instead (svdf_rank_eval_positions_cand)");
        EXPECT(refused([&] { rank_negs_build(1, p0, pos, b999, ban.data(), 1200, 101, L); }).empty());   // without positives nothing is drawn
        // avail * 64 >= num_item: 18 of 1200 left is too little even for one negative, 19 is enough
        for (unsigned b = 1000; b < 1182; b++) ban.push_back(b);
        const int64_t b1181[2] = {0, 1181}, b1180[2] = {0, 1180};
        EXPECT(refused([&] { rank_negs_build(1, p1, pos, b1181, ban.data(), 1200, 1, L); }) ==
               "rank_eval: section 0 leaves 18 items to draw 1 negatives from 1200; list its candidates instead (svdf_rank_eval_positions_cand)");
        EXPECT(refused([&] { rank_negs_build(1, p1, pos, b1180, ban.data(), 1200, 1, L); }).empty());
        std::vector<int> neg(1);
        rank_negs_host(1, p1, pos, b1180, ban.data(), 1200, 1, 5, neg.data());
        EXPECT(neg[0] >= 1181 && neg[0] < 1200);
        EXPECT(refused([&] { rank_negs_build(0, nullptr, nullptr, nullptr, nullptr, 10, 1, L); }).empty());
        EXPECT(L.ranked.empty() && L.first.size() == 1 && L.ex_first.size() == 1);
        rank_negs_host(0, nullptr, nullptr, nullptr, nullptr, 10, 1, 5, nullptr);
        std::vector<int> big(4096);
        rank_negs_host(1, p1, pos, nullptr, nullptr, 9000, 4096, 1, big.data());
        EXPECT(std::set<int>(big.begin(), big.end()).size() == 4096 && !std::set<int>(big.begin(), big.end()).count(0));
    }
    // ---- refusals, in svdf_rank_eval_positions' words and order
    {
        RankNegsLists L;
        const unsigned c2[2] = {3, 9}, cbad[2] = {3, 10}, chuge[2] = {4000000000u, 3};
        const int64_t p[3] = {0, 1, 2}, pdec[3] = {0, 2, 1}, pneg[3] = {-1, 1, 2}, none[3] = {0, 0, 0};
        const unsigned pos[2] = {4, 5}, prep[2] = {4, 4}, pban[2] = {4, 9};
        const int64_t pp[3] = {0, 0, 2};
        auto build = [&](const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg = 2) {
            return refused([&] { rank_negs_build(2, pos_ptr, pos_item, ban_ptr, ban_item, 10, num_neg, L); });
        };
        EXPECT(build(p, pos, p, c2).empty());
        EXPECT(build(p, pos, nullptr, nullptr).empty());
        EXPECT(build(p, pos, p, c2, 0) == "rank_eval: num_neg must be between 1 and 4096");
        EXPECT(build(p, pos, p, c2, 4097) == "rank_eval: num_neg must be between 1 and 4096");
        EXPECT(build(nullptr, pos, p, c2) == "rank_eval: bad arguments");
        EXPECT(build(pneg, pos, p, c2) == "rank_eval: pos_ptr must start at >= 0");
        EXPECT(build(pdec, pos, p, c2) == "rank_eval: pos_ptr must not decrease");
        EXPECT(build(p, nullptr, p, c2) == "rank_eval: pos_item is missing");
        EXPECT(build(p, pos, pneg, c2) == "rank_eval: ban_ptr must start at >= 0");
        EXPECT(build(p, pos, pdec, c2) == "rank_eval: ban_ptr must not decrease");
        EXPECT(build(p, pos, p, nullptr) == "rank_eval: ban_item is missing");
        EXPECT(build(p, pos, p, cbad) == "sample item index exceed bound");
        EXPECT(build(p, pos, p, chuge) == "sample item index exceed bound");
        EXPECT(build(none, pos, p, cbad) == "sample item index exceed bound");   // a section without positives: its ids are still validated
        EXPECT(build(pp, prep, p, c2) == "rank_eval: a positive item is repeated inside a section");
        EXPECT(build(p, prep, p, c2).empty());   // the same id in two sections is no repeat
        EXPECT(build(pp, pban, p, c2) == "each pos sample item can not occur in baned sample list");
        const unsigned pother[2] = {9, 4}, posbad[2] = {4, 10};
        EXPECT(build(p, pother, p, c2).empty());   // ... nor a ban of another section
        EXPECT(build(p, posbad, p, c2) == "sample item index exceed bound");
        EXPECT(build(p, pos, p, c2, 5) ==
               "rank_eval: section 0 leaves 8 items to draw 5 negatives from 10; list its candidates instead (svdf_rank_eval_positions_cand)");
        EXPECT(refused([&] { rank_negs_build(2, p, pos, p, c2, 0, 1, L); }) == "rank_eval: bad arguments");
        const unsigned p4[4] = {4, 4, 10, 3};
        const int64_t pp4[4] = {0, 2, 3, 4}, none4[4] = {0, 0, 0, 0};   // section 0 repeats a positive, section 1 is out of bound: the first section's refusal
        for (int threads : {1, 2, 3})
            EXPECT(refused([&] { rank_negs_build(3, pp4, p4, none4, nullptr, 10, 2, L, threads); }) == "rank_eval: a positive item is repeated inside a section");
        int out[4];
        EXPECT(refused([&] { rank_negs_host(2, p, pos, p, c2, 10, 2, 1, nullptr); }) == "rank_eval: bad arguments");
        EXPECT(refused([&] { rank_negs_host(2, p, pos, p, c2, 10, 2, 1, out); }).empty());
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

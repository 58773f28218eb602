// check_rankrows_lists.cpp -- the host-only part of the row lists of the live-model ranking calls: the feedback lists of the _fb calls and
// the USER lines of the _lines calls (svdfeature_amd/csrc/svdf_rankrows_lists.h: validation, the check of a side table's child ids, the cut
// of a piece at the entry budget, the words a piece uploads, the contiguous copy of a subset of sections) as a stand-alone program, meant
// to be built with a sanitizer:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Isvdfeature_amd/csrc tools/check_rankrows_lists.cpp -o tools/check_rankrows_lists && tools/check_rankrows_lists
// For either kind: ragged, empty and long lists with repeated ids and any float value, every refusal in its published words, pieces under
// small and large budgets, the packed words of every piece, and the subset copies a relisting call makes.  Exit status 0 and "ok" when
// all holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <stdexcept>

#include "svdf_rankrows_lists.h"

namespace svdf {
[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }
}  // namespace svdf

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED line %d (%s): %s\n", __LINE__, kind_name, #cond); failures++; } } while (0)

template <typename F>
static std::string refused(F f) {
    try { f(); } catch (const std::runtime_error &e) { return e.what(); }
    return "";
}

static svdf::RankList list_of(const int64_t *ptr, const unsigned *index, const float *value) {
    svdf::RankList L;
    L.ptr = ptr; L.index = index; L.value = value;
    return L;
}

// one kind of list: its descriptor, its id space, the shape of the random lists and the words of its messages
struct Kind {
    const svdf::RankListKind &K;
    const char *name;
    long num_id;
    unsigned seed;
    long max_len, empty_at, long_at;   // 0 .. max_len entries a list, an empty list, one list of 300 entries
    bool one_list_a_piece;             // under a budget of 1: every list has entries, bar one
    const char *bound, *decrease_eval, *start_topn, *arrays_topn, *arrays_eval, *ptr_eval, *entries_topn;
};

static bool same_bits(const float *a, const float *b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(float)) == 0; }

// the subset copy of sections again[0 .. A) against the lists built directly from the chosen sections, values by their bits
static void check_subset(const char *kind_name, const svdf::RankList &L, const std::vector<long> &again) {
    using namespace svdf;
    const long A = (long)again.size();
    RankListCopy got;
    got.ptr.assign(3, 77); got.index.assign(5, 9u); got.value.assign(5, 1.0f);   // whatever it held before is gone
    rank_list_subset(again.data(), A, L, got);
    std::vector<int64_t> ptr(1, 0);
    std::vector<unsigned> idx;
    std::vector<float> val;
    for (long s : again) {
        for (int64_t j = L.ptr[s]; j < L.ptr[s + 1]; j++) { idx.push_back(L.index[j]); val.push_back(L.value[j]); }
        ptr.push_back((int64_t)idx.size());
    }
    EXPECT(got.ptr == ptr && got.index == idx && got.value.size() == val.size() && same_bits(got.value.data(), val.data(), val.size()));
    EXPECT(got.ptr[0] == 0 && (long)got.ptr.size() == A + 1);   // a copy starts at entry 0 wherever the lists did
    // ... and it packs as the chosen sections would, one piece
    const RankList C = got.view();
    std::vector<int> words(rank_list_words(0, A, C));
    rank_list_pack(0, A, C, words.data());
    EXPECT(words.size() == (size_t)A + 1 + 2 * idx.size() && words[0] == 0 && words[(size_t)A] == (int)idx.size());
    for (size_t q = 0; q < idx.size(); q++) {
        EXPECT((unsigned)words[(size_t)A + 1 + q] == idx[q]);
        EXPECT(std::memcmp(&words[(size_t)A + 1 + idx.size() + q], &val[q], 4) == 0);
    }
}

static void check_kind(const Kind &k) {
    using namespace svdf;
    const char *kind_name = k.name;
    const RankListKind &K = k.K;
    const long nid = k.num_id;
    std::mt19937 rng(k.seed);
    // ---- random ragged lists with repeated ids, an empty list, one list of 300 entries, values of every kind
    const long S = 150;
    std::vector<unsigned> idx;
    std::vector<float> val;
    std::vector<int64_t> ptr((size_t)S + 1, 0);
    for (long s = 0; s < S; s++) {
        long n = (long)(rng() % (unsigned)(k.max_len + 1));
        if (s == k.empty_at) n = 0;
        if (s == k.long_at) n = 300;
        for (long j = 0; j < n; j++) {
            const unsigned f = (unsigned)(rng() % nid);
            idx.push_back(f);
            val.push_back((float)((int)(rng() % 2001) - 1000) / 700.0f);
            if (rng() % 5 == 0) { idx.push_back(f); val.push_back(-0.0f); }   // a repeated id
        }
        ptr[(size_t)s + 1] = (int64_t)idx.size();
    }
    val[3] = std::numeric_limits<float>::quiet_NaN();   // any float value is legal
    val[4] = std::numeric_limits<float>::infinity();
    val[6] = 1.0f + 5e-7f;
    const RankList U = list_of(ptr.data(), idx.data(), val.data());
    EXPECT(refused([&] { rank_list_validate(K, "rank_eval", S, U, nid); }).empty());
    EXPECT(refused([&] { rank_list_validate(K, "rank_topn", S - 7, list_of(ptr.data() + 7, idx.data(), val.data()), nid); }).empty());   // lists that start past entry 0
    // ---- pieces: whole sections, in order, all of them, within the budget unless one section alone exceeds it; the packed words are the lists
    for (int64_t budget : {(int64_t)1, (int64_t)7, (int64_t)100, (int64_t)299, (int64_t)300, (int64_t)100000, (int64_t)1 << 40}) {
        long s0 = 0, pieces = 0;
        while (s0 < S) {
            const long cap = std::min(S, s0 + 64);   // the caller's own cut
            const long s1 = rank_list_piece(K, "rank_topn", s0, cap, U, budget);
            EXPECT(s1 > s0 && s1 <= cap);
            EXPECT(s1 == s0 + 1 || ptr[(size_t)s1] - ptr[(size_t)s0] <= budget);
            EXPECT(s1 == cap || ptr[(size_t)s1 + 1] - ptr[(size_t)s0] > budget);   // ... and no shorter than it must be
            std::vector<int> words(rank_list_words(s0, s1, U));
            rank_list_pack(s0, s1, U, words.data());
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
        if (budget == 1 && k.one_list_a_piece) EXPECT(pieces == S);
        if (budget == 1) EXPECT(pieces > S / 2);   // only lists of no or one entry share a piece
    }
    // ---- no sections, all lists empty without arrays
    {
        const int64_t zeros[3] = {0, 0, 0};
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 0, RankList(), nid); }).empty());
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(zeros, nullptr, nullptr), nid); }).empty());
        EXPECT(rank_list_piece(K, "rank_eval", 0, 2, list_of(zeros, nullptr, nullptr), 1) == 2 && rank_list_words(0, 2, list_of(zeros, nullptr, nullptr)) == 3);
        int words[3] = {-1, -1, -1};
        rank_list_pack(0, 2, list_of(zeros, nullptr, nullptr), words);
        EXPECT(words[0] == 0 && words[1] == 0 && words[2] == 0);
        check_subset(kind_name, list_of(zeros, nullptr, nullptr), {0, 1});
    }
    // ---- refusals
    {
        const unsigned u2[2] = {3, (unsigned)nid - 1}, ubad[2] = {3, (unsigned)nid}, uhuge[2] = {4000000000u, 3};
        const float v2[2] = {0.5f, -2.0f};
        const int64_t p[3] = {0, 1, 2}, pdec[3] = {0, 2, 1}, pneg[3] = {-1, 1, 2};
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(p, u2, v2), nid); }).empty());
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(p, ubad, v2), nid); }) == k.bound);
        EXPECT(refused([&] { rank_list_validate(K, "rank_topn", 2, list_of(p, uhuge, v2), nid); }) == k.bound);
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(pdec, u2, v2), nid); }) == k.decrease_eval);
        EXPECT(refused([&] { rank_list_validate(K, "rank_topn", 2, list_of(pneg, u2, v2), nid); }) == k.start_topn);
        EXPECT(refused([&] { rank_list_validate(K, "rank_topn", 2, list_of(p, nullptr, v2), nid); }) == k.arrays_topn);
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(p, u2, nullptr), nid); }) == k.arrays_eval);
        EXPECT(refused([&] { rank_list_validate(K, "rank_eval", 2, list_of(nullptr, u2, v2), nid); }) == k.ptr_eval);
        const int64_t big[2] = {0, (int64_t)1 << 30};
        EXPECT(refused([&] { rank_list_piece(K, "rank_topn", 0, 1, list_of(big, nullptr, nullptr), 100); }) == k.entries_topn);
    }
    // ---- the subset copy: one section, all of them, every other one, empty lists at the ends, lists that start past entry 0
    {
        std::vector<long> all((size_t)S), odd, even, ends = {k.empty_at, k.long_at - 1, k.long_at, S - 1};
        for (long s = 0; s < S; s++) { all[(size_t)s] = s; (s % 2 ? odd : even).push_back(s); }
        std::sort(ends.begin(), ends.end());
        for (long s : {0L, 1L, k.empty_at, k.long_at, S - 1}) check_subset(kind_name, U, {s});   // A = 1
        check_subset(kind_name, U, all);                                                       // A = S
        check_subset(kind_name, U, odd);
        check_subset(kind_name, U, even);
        check_subset(kind_name, U, ends);
        check_subset(kind_name, U, {k.empty_at});
        check_subset(kind_name, U, {k.empty_at, 60, 61, k.empty_at + 100 < S ? k.empty_at + 100 : S - 1});   // an empty list at the start
        // empty lists at both ends of the choice, and of the call: sections 0 and S - 1 emptied in a copy of the pointers
        std::vector<int64_t> hollow(ptr);
        hollow[1] = hollow[0];
        hollow[(size_t)S - 1] = hollow[(size_t)S];
        const RankList H = list_of(hollow.data(), idx.data(), val.data());
        check_subset(kind_name, H, {0, 1, 2, S - 2, S - 1});
        check_subset(kind_name, H, {0, S - 1});
        check_subset(kind_name, H, all);
        // lists that start past entry 0: the last S - 7 sections, whose ptr[0] > 0
        const RankList P7 = list_of(ptr.data() + 7, idx.data(), val.data());
        EXPECT(P7.ptr[0] > 0);
        std::vector<long> some;
        for (long s = 0; s < S - 7; s += 3) some.push_back(s);
        check_subset(kind_name, P7, some);
        check_subset(kind_name, P7, {0});
        check_subset(kind_name, P7, {S - 8});
    }
}

int main() {
    using namespace svdf;
    const char *kind_name = "children";
    check_kind(Kind{RANK_FB_LISTS, "feedback lists", 90, 11, 40, 20, 33, true, "ufeedback id exceed bound", "rank_eval: fb_ptr must not decrease",
                    "rank_topn: fb_ptr must start at >= 0", "rank_topn: fb_index / fb_value is missing", "rank_eval: fb_index / fb_value is missing",
                    "rank_eval: fb_ptr is missing", "rank_topn: one section with more than 2^30 feedback entries"});
    check_kind(Kind{RANK_USER_LINES, "USER lines", 200, 13, 6, 5, 40, false, "user feature index exceed bound", "rank_eval: ul_ptr must not decrease",
                    "rank_topn: ul_ptr must start at >= 0", "rank_topn: ul_index / ul_value is missing", "rank_eval: ul_index / ul_value is missing",
                    "rank_eval: ul_ptr is missing", "rank_topn: one section with more than 2^30 line entries"});
    // ---- a side table's child ids against their id space; an empty table
    {
        const long nu = 200;
        const std::vector<unsigned> kids = {0, 199, 7, 7}, out = {0, 200};
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", kids, nu); }).empty());
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", std::vector<unsigned>(), nu); }).empty());
        EXPECT(refused([&] { rank_lines_check_children("rank_eval", "feature_user", out, nu); }) == "rank_eval: feature_user: child index exceed bound");
        EXPECT(refused([&] { rank_lines_check_children("rank_topn", "feature_item", kids, 199); }) == "rank_topn: feature_item: child index exceed bound");
    }
    std::printf(failures ? "%d checks FAILED\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

// svdf_rankrows_lists.h -- the host-only part of what the sections of a live-model ranking call score with (DESIGN.md sections 6y, 6z): the
// feedback lists of the _fb calls and the USER lines of the _lines calls as ONE ragged list type -- validation, the cut of a piece at the
// entry budget, the words a piece uploads, the contiguous copy of a subset of sections -- the check of a side table's child ids, and the
// value the ranking paths hand on in place of loose pointers.  Plain C++ without a device call, so that tools/check_rankrows_lists.cpp can
// run it under a sanitizer.
#ifndef SVDF_RANKROWS_LISTS_H_
#define SVDF_RANKROWS_LISTS_H_

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

// a ragged list per section: section s carries the (id, value) entries [ptr[s], ptr[s + 1]) in the caller's order; absent when ptr == nullptr
struct RankList {
    const int64_t *ptr = nullptr;
    const unsigned *index = nullptr;
    const float *value = nullptr;
};

// the two kinds of list, by the names their messages carry
struct RankListKind {
    const char *ptr_name, *arrays_name;   // the caller's arrays
    const char *bound;                    // an id at or above its id space: the ranker's message, bare
    const char *entries;                  // "... 2^30 <entries> entries"
};
constexpr RankListKind RANK_FB_LISTS = {"fb_ptr", "fb_index / fb_value", "ufeedback id exceed bound", "feedback"};     // ids below num_ufeedback
constexpr RankListKind RANK_USER_LINES = {"ul_ptr", "ul_index / ul_value", "user feature index exceed bound", "line"};   // ids below num_user

// Everything the calls refuse about the lists themselves (whether a trainer takes lists at all is the engine's business); `who` is the
// prefix of the messages, "rank_eval" or "rank_topn".  Empty lists, repeated ids and any float value are legal.
static inline void rank_list_validate(const RankListKind &K, const char *who, long S, const RankList &L, long num_id) {
    const std::string w(who);
    if (S <= 0) return;
    if (!L.ptr) fail(w + ": " + K.ptr_name + " is missing");
    if (L.ptr[0] < 0) fail(w + ": " + K.ptr_name + " must start at >= 0");
    for (long s = 0; s < S; s++)
        if (L.ptr[s + 1] < L.ptr[s]) fail(w + ": " + K.ptr_name + " must not decrease");
    if (L.ptr[S] != 0 && !(L.index && L.value)) fail(w + ": " + K.arrays_name + " is missing");
    for (int64_t j = L.ptr[0]; j < L.ptr[S]; j++)
        if ((long)L.index[j] >= num_id) fail(K.bound);
}

// a side table's child ids against their id space (the table loader refuses them too; the calls check once more, the tables are small)
static inline void rank_lines_check_children(const char *who, const char *table, const std::vector<unsigned> &child, long num_id) {
    for (unsigned c : child)
        if ((long)c >= num_id) fail(std::string(who) + ": " + table + ": child index exceed bound");
}

// The sections [s0, s1) of a piece cut so that its entries stay within `budget` (at least one section, and fewer than 2^30 entries unless
// one section alone holds more, which is refused).  Returns the new end.
static inline long rank_list_piece(const RankListKind &K, const char *who, long s0, long s1, const RankList &L, int64_t budget) {
    if (budget > ((int64_t)1 << 30) - 1) budget = ((int64_t)1 << 30) - 1;
    long e = s0 + 1;
    while (e < s1 && L.ptr[e + 1] - L.ptr[s0] <= budget) e++;
    if (L.ptr[e] - L.ptr[s0] >= (int64_t)1 << 30) fail(std::string(who) + ": one section with more than 2^30 " + K.entries + " entries");
    return e;
}

// words a piece adds to its upload: p0[nsec + 1] | index[n] | value[n] (the values' bits), every offset relative to the piece's first entry
static inline size_t rank_list_words(long s0, long s1, const RankList &L) { return (size_t)(s1 - s0) + 1 + 2 * (size_t)(L.ptr[s1] - L.ptr[s0]); }
static inline void rank_list_pack(long s0, long s1, const RankList &L, int *out) {
    const size_t nsec = (size_t)(s1 - s0), n = (size_t)(L.ptr[s1] - L.ptr[s0]);
    for (long s = s0; s <= s1; s++) out[s - s0] = (int)(L.ptr[s] - L.ptr[s0]);
    if (n) {
        std::memcpy(out + nsec + 1, L.index + L.ptr[s0], n * sizeof(int));
        std::memcpy(out + nsec + 1 + n, L.value + L.ptr[s0], n * sizeof(int));
    }
}

// a list that owns its arrays
struct RankListCopy {
    std::vector<int64_t> ptr;
    std::vector<unsigned> index;
    std::vector<float> value;
    RankList view() const { return RankList{ptr.data(), index.data(), value.data()}; }
};

// the lists of the sections again[0 .. A) (ascending section indices of L), one behind the other from entry 0
static inline void rank_list_subset(const long *again, long A, const RankList &L, RankListCopy &out) {
    out.ptr.assign((size_t)A + 1, 0);
    out.index.clear();
    out.value.clear();
    for (long a = 0; a < A; a++) {
        const long s = again[a];
        if (L.ptr[s + 1] > L.ptr[s]) {
            out.index.insert(out.index.end(), L.index + L.ptr[s], L.index + L.ptr[s + 1]);
            out.value.insert(out.value.end(), L.value + L.ptr[s], L.value + L.ptr[s + 1]);
        }
        out.ptr[(size_t)a + 1] = (int64_t)out.index.size();
    }
}

// What the sections of a call score with: a user each (nullptr where USER lines are given: the kernels do not read it then), the row the
// device builds from their feedback lists and USER lines, the prepared item side of a trainer with a feature_item table (nullptr: the
// model's own), and -- an item call (svdf_itemtopn.cpp) -- the [num_item][pitch] matrix the sections' query rows are gathered from.
struct RankRowSource {
    const unsigned *user = nullptr;
    RankList fb, lines;
    bool by_lines = false;   // a _lines call: the sections come without users, and lines whose ptr is missing are refused in those words
    const float *item_rows = nullptr, *item_bias = nullptr;
    const float *query_base = nullptr;
    int user_of(long s) const { return user ? (int)user[s] : 0; }   // the word a section uploads as sec_user
};

// the row lists of a piece as the tail of its upload: the reserve term, and where the two lists begin (0 where there is none)
struct RankRowsAt { size_t fb = 0, ul = 0; };
static inline size_t rank_rows_words(const RankRowSource &R, long s0, long s1) {
    return (R.fb.ptr ? rank_list_words(s0, s1, R.fb) : 0) + (R.lines.ptr ? rank_list_words(s0, s1, R.lines) : 0);
}

// The sections again[0 .. A) of a call that its prefilter did not certify, as contiguous copies of what they bring: ids (users or query
// items), the validated ban lists and the row lists.  `rows` scores with the copies and the item side of the call.
struct RankRelist {
    std::vector<long> again;
    std::vector<unsigned> ids;
    std::vector<int64_t> ban_first;
    std::vector<int> ban_ids;
    RankListCopy fb, lines;
    RankRowSource rows;

    RankRelist(const std::vector<long> &sections, const RankRowSource &R, const std::vector<int64_t> &first, const std::vector<int> &bans)
        : again(sections), ids(sections.size(), 0u), ban_first(sections.size() + 1, 0), rows(R) {
        const long A = (long)again.size();
        for (long a = 0; a < A; a++) {
            const size_t s = (size_t)again[(size_t)a];
            if (R.user) ids[(size_t)a] = R.user[s];
            ban_ids.insert(ban_ids.end(), bans.begin() + (long)first[s], bans.begin() + (long)first[s + 1]);
            ban_first[(size_t)a + 1] = (int64_t)ban_ids.size();
        }
        if (R.user) rows.user = ids.data();
        if (R.fb.ptr) { rank_list_subset(again.data(), A, R.fb, fb); rows.fb = fb.view(); }
        if (R.lines.ptr) { rank_list_subset(again.data(), A, R.lines, lines); rows.lines = lines.view(); }
    }
    RankRelist(const RankRelist &) = delete;   // `rows` points into this object
    RankRelist &operator=(const RankRelist &) = delete;

    // section again[a]'s results src[src_at(a) .. src_at(a + 1)) to dst + dst_at(again[a])
    template <typename T, typename SrcAt, typename DstAt>
    void scatter(const T *src, SrcAt src_at, T *dst, DstAt dst_at) const {
        for (long a = 0; a < (long)again.size(); a++) std::copy(src + src_at(a), src + src_at(a + 1), dst + dst_at(again[(size_t)a]));
    }
};

}  // namespace svdf
#endif

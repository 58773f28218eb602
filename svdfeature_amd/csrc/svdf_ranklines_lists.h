// svdf_ranklines_lists.h -- the host-only part of the USER lines of svdf_rank_eval*_lines / svdf_rank_topn_lines: their
// validation, the check of a side table's child ids, the cut of a piece at the entry budget and the words a piece uploads.  Plain C++
// without a device call, so that tools/check_ranklines_lists.cpp can run it under a sanitizer.
#ifndef SVDF_RANKLINES_LISTS_H_
#define SVDF_RANKLINES_LISTS_H_

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

// the USER lines of a call: section s carries the (id, value) entries [ptr[s], ptr[s + 1]) in line order
struct RankLines {
    const int64_t *ptr = nullptr;
    const unsigned *index = nullptr;
    const float *value = nullptr;
};

// Everything the _lines calls refuse about the lines themselves; `who` is the prefix of the messages, "rank_eval" or "rank_topn".  An id
// must be below num_user (the ranker's message, bare).  Empty lines, repeated ids and any float value are legal.
static inline void rank_lines_validate(const char *who, long S, const RankLines &U, long num_user) {
    const std::string w(who);
    if (S <= 0) return;
    if (!U.ptr) fail(w + ": ul_ptr is missing");
    if (U.ptr[0] < 0) fail(w + ": ul_ptr must start at >= 0");
    for (long s = 0; s < S; s++)
        if (U.ptr[s + 1] < U.ptr[s]) fail(w + ": ul_ptr must not decrease");
    if (U.ptr[S] != 0 && !(U.index && U.value)) fail(w + ": ul_index / ul_value is missing");
    for (int64_t j = U.ptr[0]; j < U.ptr[S]; j++)
        if ((long)U.index[j] >= num_user) fail("user feature index exceed bound");
}

// a side table's child ids against their id space (the table loader refuses them too; the calls check once more, the tables are small)
static inline void rank_lines_check_children(const char *who, const char *table, const std::vector<unsigned> &child, long num_id) {
    for (unsigned c : child)
        if ((long)c >= num_id) fail(std::string(who) + ": " + table + ": child index exceed bound");
}

// The sections [s0, s1) of a piece cut so that its line entries stay within `budget` (at least one section, and fewer than 2^30 entries
// unless one section alone holds more, which is refused).  Returns the new end.
static inline long rank_lines_piece(const char *who, long s0, long s1, const int64_t *ul_ptr, int64_t budget) {
    if (budget > ((int64_t)1 << 30) - 1) budget = ((int64_t)1 << 30) - 1;
    long e = s0 + 1;
    while (e < s1 && ul_ptr[e + 1] - ul_ptr[s0] <= budget) e++;
    if (ul_ptr[e] - ul_ptr[s0] >= (int64_t)1 << 30) fail(std::string(who) + ": one section with more than 2^30 line entries");
    return e;
}

// words a piece adds to its upload: ul_p0[nsec + 1] | ul_index[n] | ul_value[n] (the values' bits)
static inline size_t rank_lines_words(long s0, long s1, const int64_t *ul_ptr) { return (size_t)(s1 - s0) + 1 + 2 * (size_t)(ul_ptr[s1] - ul_ptr[s0]); }
static inline void rank_lines_pack(long s0, long s1, const RankLines &U, int *out) {
    const size_t nsec = (size_t)(s1 - s0), n = (size_t)(U.ptr[s1] - U.ptr[s0]);
    for (long s = s0; s <= s1; s++) out[s - s0] = (int)(U.ptr[s] - U.ptr[s0]);
    if (n) {
        std::memcpy(out + nsec + 1, U.index + U.ptr[s0], n * sizeof(int));
        std::memcpy(out + nsec + 1 + n, U.value + U.ptr[s0], n * sizeof(int));
    }
}

}  // namespace svdf
#endif

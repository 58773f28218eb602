// svdf_rankfb_lists.h -- the host-only part of the feedback lists of svdf_rank_eval*_fb / svdf_rank_topn_fb: their
// validation, the cut of a piece at the feedback budget and the words a piece uploads.  Plain C++ without a device call, so that
// tools/check_rankfb_lists.cpp can run it under a sanitizer.
#ifndef SVDF_RANKFB_LISTS_H_
#define SVDF_RANKFB_LISTS_H_

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

// Everything the _fb calls refuse about the feedback lists themselves (whether a trainer takes lists at all is the engine's business);
// `who` is the prefix of the messages, "rank_eval" or "rank_topn".  Section s carries the entries [fb_ptr[s], fb_ptr[s + 1]); an id must be
// below num_ufeedback (the ranker's message).  Empty lists, repeated ids and any float value are legal.
static inline void rank_fb_validate(const char *who, long S, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, long num_ufeedback) {
    const std::string w(who);
    if (S <= 0) return;
    if (!fb_ptr) fail(w + ": fb_ptr is missing");
    if (fb_ptr[0] < 0) fail(w + ": fb_ptr must start at >= 0");
    for (long s = 0; s < S; s++)
        if (fb_ptr[s + 1] < fb_ptr[s]) fail(w + ": fb_ptr must not decrease");
    if (fb_ptr[S] != 0 && !(fb_index && fb_value)) fail(w + ": fb_index / fb_value is missing");
    for (int64_t j = fb_ptr[0]; j < fb_ptr[S]; j++)
        if ((long)fb_index[j] >= num_ufeedback) fail("ufeedback id exceed bound");
}

// The sections [s0, s1) of a piece cut so that its feedback entries stay within `budget` (at least one section, and fewer than 2^30
// entries unless one section alone holds more, which is refused).  Returns the new end.
static inline long rank_fb_piece(const char *who, long s0, long s1, const int64_t *fb_ptr, int64_t budget) {
    if (budget > ((int64_t)1 << 30) - 1) budget = ((int64_t)1 << 30) - 1;
    long e = s0 + 1;
    while (e < s1 && fb_ptr[e + 1] - fb_ptr[s0] <= budget) e++;
    if (fb_ptr[e] - fb_ptr[s0] >= (int64_t)1 << 30) fail(std::string(who) + ": one section with more than 2^30 feedback entries");
    return e;
}

// words a piece adds to its upload: fb_p0[nsec + 1] | fb_index[n] | fb_value[n] (the values' bits)
static inline size_t rank_fb_words(long s0, long s1, const int64_t *fb_ptr) { return (size_t)(s1 - s0) + 1 + 2 * (size_t)(fb_ptr[s1] - fb_ptr[s0]); }
static inline void rank_fb_pack(long s0, long s1, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, int *out) {
    const size_t nsec = (size_t)(s1 - s0), n = (size_t)(fb_ptr[s1] - fb_ptr[s0]);
    for (long s = s0; s <= s1; s++) out[s - s0] = (int)(fb_ptr[s] - fb_ptr[s0]);
    if (n) {
        std::memcpy(out + nsec + 1, fb_index + fb_ptr[s0], n * sizeof(int));
        std::memcpy(out + nsec + 1 + n, fb_value + fb_ptr[s0], n * sizeof(int));
    }
}

}  // namespace svdf
#endif

// svdf_foldin_lists.h -- the host-only part of svdf_fold_in: everything the call refuses about its arguments, and
// the one packed buffer the kernel reads.  Plain C++ without a device call.  The rule is stated in full in include/svdfeature_amd.h.
#ifndef SVDF_FOLDIN_LISTS_H_
#define SVDF_FOLDIN_LISTS_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace svdf {

[[noreturn]] void fail(const std::string &msg);

constexpr int FOLD_IN_MAX_FACTOR = 128;

// Nothing is written anywhere before all of it holds.  Returns the number of ratings, ptr[S] - ptr[0].
static inline int64_t fold_in_validate(long S, const unsigned *user, const int64_t *ptr, const unsigned *item, const float *label, float reg, int write,
                                       const float *rows_out, long num_user, long num_item) {
    auto need = [](bool ok, const char *msg) { if (!ok) fail(msg); };
    need(std::isfinite(reg) && reg > 0.0f, "fold_in: reg must be finite and > 0");
    need(S >= 0 && (S == 0 || (user && ptr && rows_out)), "fold_in: bad arguments");
    if (S == 0) return 0;
    need(ptr[0] >= 0, "fold_in: ptr must start at >= 0");
    for (long s = 0; s < S; s++) need(ptr[s + 1] >= ptr[s], "fold_in: ptr must not decrease");
    need(ptr[S] == ptr[0] || (item && label), "fold_in: bad arguments");
    for (long s = 0; s < S; s++) need((long)user[s] < num_user, "user feature index exceed bound");
    for (int64_t j = ptr[0]; j < ptr[S]; j++) need((long)item[j] < num_item, "sample item index exceed bound");
    if (write) {
        std::vector<unsigned char> seen((size_t)num_user, 0);
        for (long s = 0; s < S; s++) {
            if (seen[user[s]]) fail("fold_in: user " + std::to_string(user[s]) + " is written by two sections");
            seen[user[s]] = 1;
        }
    }
    return ptr[S] - ptr[0];
}

// The upload, in 8-byte words: ptr - ptr[0] [S + 1] | user [S] | item [n] | label [n], the 4-byte arrays back to back
struct FoldInPack {
    std::vector<int64_t> words;
    size_t o_user = 0, o_item = 0, o_label = 0;   // offsets in 4-byte units from the start
};
static inline void fold_in_pack(long S, const unsigned *user, const int64_t *ptr, const unsigned *item, const float *label, int64_t n, FoldInPack &out) {
    out.o_user = 2 * ((size_t)S + 1);
    out.o_item = out.o_user + (size_t)S;
    out.o_label = out.o_item + (size_t)n;
    out.words.assign((out.o_label + (size_t)n + 1) / 2, 0);
    for (long s = 0; s <= S; s++) out.words[(size_t)s] = ptr[s] - ptr[0];
    char *base = reinterpret_cast<char *>(out.words.data());
    std::memcpy(base + 4 * out.o_user, user, (size_t)S * 4);
    if (n > 0) {
        std::memcpy(base + 4 * out.o_item, item + ptr[0], (size_t)n * 4);
        std::memcpy(base + 4 * out.o_label, label + ptr[0], (size_t)n * 4);
    }
}

}  // namespace svdf
#endif

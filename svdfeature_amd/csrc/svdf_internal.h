// svdf_internal.h -- helpers shared by the translation units of the host engine (svdf_engine / _config / _model / _sched /
// _dataset / _window .cpp).  Not part of the boundary; include/svdfeature_amd.h is.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "svdf_engine.h"

namespace svdf {

static inline void check(bool ok, const char *msg) { if (!ok) fail(msg); }
#define HIPCHECK(call)                                                                           \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #call); \
    } while (0)

// The first real HIP call initialises the ROCm runtime, which disturbs libc's rand() state (tools/check_hip_init_rand.cpp);
// runtime start-up runs on a scratch PRNG state and the caller's state is put back exactly.
struct RandStateGuard {
    char scratch[256];
    char *old;
    RandStateGuard() { old = initstate(1u, scratch, sizeof(scratch)); }
    ~RandStateGuard() { if (old) setstate(old); }
};
struct ScopedNs {   // host-side time accounting (SVDF_PROFILE=1)
    int64_t &acc;
    std::chrono::steady_clock::time_point t0;
    explicit ScopedNs(int64_t &a) : acc(a), t0(std::chrono::steady_clock::now()) {}
    ~ScopedNs() { acc += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};

// config keys of SVDTrainParam / SVDModelParam (svdf_config.cpp: one table row per key)
void config_set_train_param(TrainParam &p, const char *name, const char *val);
void config_set_model_param(ModelParam &p, const char *name, const char *val);

// The window rule evaluated on the windows AS CUT (svdf_wunit.cpp: wseq_windows_actual).  The per-pass rules bound what a
// row meets per window on average (c / W); the windows are cut at equal positions n w / W, so on a file sorted by item, or one that arrives in
// bursts, one window can hold all of a row's updates.  A class of shared rows keeps two quantities on the actual windows: the mean over its
// entries of min(count of the entry's row in its window, sub) (sub 0: the count) at `target`, and the most updates of one row in one window at
// `cap`.  target <= 0 / cap <= 0: not checked.
struct WseqClass {
    long num_id;     // ids of the class are 0 .. num_id - 1
    double target;
    long cap;
    int sub;
};
class WseqCounter {   // one scan: the caller walks the windows in order and adds every entry of the window's rows
 public:
    explicit WseqCounter(const std::vector<WseqClass> &classes) {
        for (const WseqClass &k : classes) { cls_.push_back(Class{k, {}, {}, 0.0, 0, 0}); cls_.back().stamp.assign((size_t)k.num_id, -1); cls_.back().count.assign((size_t)k.num_id, 0); }
    }
    void begin_scan() { for (Class &c : cls_) { std::fill(c.stamp.begin(), c.stamp.end(), -1); c.sum = 0.0; c.entries = 0; c.worst = 0; } }
    void begin_window(long w) { w_ = (int)w; }
    void add(int k, unsigned id) {
        Class &c = cls_[(size_t)k];
        if (c.stamp[id] != w_) { c.stamp[id] = w_; c.count[id] = 0; }
        const int v = ++c.count[id];
        c.worst = std::max<long>(c.worst, v);
        // sum over a row's v entries of min(v, sub) = v min(v, sub): what the v-th entry adds to it
        c.sum += (c.k.sub == 0 || v <= c.k.sub) ? 2.0 * (double)v - 1.0 : (double)c.k.sub;
        c.entries++;
    }
    // how far the worst class is over its bounds, slack included, as a fraction num / den (<= 1: every bound holds)
    void excess(double slack, double &num, double &den) const {
        num = 0.0; den = 1.0;
        auto take = [&](double a, double b) { if (a / b > num / den) { num = a; den = b; } };
        for (const Class &c : cls_) {
            if (c.k.target > 0.0 && c.entries > 0) take(c.sum / (double)c.entries, c.k.target * slack);
            if (c.k.cap > 0) take((double)c.worst, (double)c.k.cap * slack);
        }
    }
 private:
    struct Class { WseqClass k; std::vector<int> stamp, count; double sum; long entries, worst; };
    std::vector<Class> cls_;
    int w_ = 0;
};
// More windows at equal positions until every class holds on the windows [n w / W, n (w + 1) / W): scan(b0, b1, counter) adds the entries of the
// file rows [b0, b1).  At most `rounds` scans; then W = n (one row per window meets every bound) when last_resort, else the count reached.
template <typename Scan>
long wseq_windows_actual(long W, long n, const std::vector<WseqClass> &classes, double slack, int rounds, bool last_resort, Scan scan) {
    if (n <= 0) return W;
    WseqCounter C(classes);
    for (int round = 0; round < rounds; round++) {
        C.begin_scan();
        for (long w = 0; w < W; w++) { C.begin_window(w); scan(n * w / W, n * (w + 1) / W, C); }
        double num, den;
        C.excess(slack, num, den);
        if (num <= den) return W;
        W = std::max<long>(W + 1, (long)std::ceil((double)W * num / den));
        if (W >= n) return n;
    }
    return last_resort ? n : W;
}
// The same search for ONE class without sub-steps (sub 0) whose entries are counted elsewhere (device columns: svdf_k_rankwin.hip): count(W, sum,
// worst) gives the sum over (row, window) of c^2 -- what WseqCounter::add's 2 v - 1 terms add up to -- and the largest c on the W windows.  The
// counter's sums are doubles of integers, so the integers give the same excess and the same W.
template <typename Count>
long wseq_windows_actual_counted(long W, long n, const WseqClass &k, long entries, double slack, int rounds, bool last_resort, Count count) {
    if (n <= 0) return W;
    for (int round = 0; round < rounds; round++) {
        unsigned long long sum = 0ull, worst = 0ull;
        count(W, sum, worst);
        double num = 0.0, den = 1.0;
        auto take = [&](double a, double b) { if (a / b > num / den) { num = a; den = b; } };
        if (k.target > 0.0 && entries > 0) take((double)sum / (double)entries, k.target * slack);
        if (k.cap > 0) take((double)(long)worst, (double)k.cap * slack);
        if (num <= den) return W;
        W = std::max<long>(W + 1, (long)std::ceil((double)W * num / den));
        if (W >= n) return n;
    }
    return last_resort ? n : W;
}

// Pointer arrays handed over by a caller are checked before anything indexes through them (the messages of dataset_from_csr /
// dataset_from_blocks): counts not negative, pointers starting at >= 0 and non-decreasing, fewer than 2^31 entries.
void validate_csr_pointers(long num_row, const int64_t *row_ptr);
void validate_block_pointers(long num_block, const int64_t *fb_ptr, const int64_t *block_row_ptr);
// the shapes the user-unit window step takes (svdf_wunit.cpp's builders fail on anything else): one user entry per row, one user per
// block / START..END span, no id twice in a row's global or item entries, no feedback id twice in a block.  Pointers must be valid.
bool wunit_rows_ok(long r0, long r1, const int64_t *row_ptr, const unsigned *feat_index, unsigned shared_from = 0xFFFFFFFFu);
bool wunit_blocks_ok(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const int64_t *block_row_ptr,
                     const int64_t *row_ptr, const unsigned *feat_index, unsigned shared_from = 0xFFFFFFFFu);
// every row of the blocks has exactly one user entry (no shared user ids).  `auto` and the staged route take the window step on user-group blocks
// only then: rows with shared ids are trained by it from resident data sets under amd:step = minibatch alone, until its
// accuracy contract has been measured on such data
bool wunit_blocks_one_user_entry(long num_block, const int64_t *block_row_ptr, const int64_t *row_ptr);

// Instances of one batch commute: sorting a batch by a key changes no bit of the result (svdf_sched.cpp)
void sort_batches(Schedule &sched, const unsigned *key);

// fn(a, b) over [0, n) in contiguous chunks on up to 16 host threads (fn must not throw)
template <typename F>
static void parallel_rows(long n, F fn) {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < (1 << 18) || hw == 1) { fn(0L, n); return; }
    std::vector<std::thread> th;
    const long chunk = (n + hw - 1) / hw;
    for (unsigned t = 0; t < hw; t++) {
        const long lo = t * chunk, hi = std::min(n, lo + chunk);
        if (lo >= hi) break;
        th.emplace_back([=]() { fn(lo, hi); });
    }
    for (auto &x : th) x.join();
}

template <typename T>
static void parallel_gather(T *dst, const T *src, const int *order, long n, long stride, long offset) {
    // dst[s] = src[order[s]*stride + offset]
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < (1 << 20) || hw == 1) {
        for (long s = 0; s < n; s++) dst[s] = src[(long)order[s] * stride + offset];
        return;
    }
    std::vector<std::thread> th;
    const long chunk = (n + hw - 1) / hw;
    for (unsigned t = 0; t < hw; t++) {
        const long a = t * chunk, b = std::min(n, a + chunk);
        if (a >= b) break;
        th.emplace_back([=]() { for (long s = a; s < b; s++) dst[s] = src[(long)order[s] * stride + offset]; });
    }
    for (auto &x : th) x.join();
}

}  // namespace svdf

// svdf_wseq_rule.h -- the window rule: into how many windows a pass is cut under `amd:step = minibatch` (DESIGN.md sections 6, 6k, 6m, 6r), and
// where a pass of user-group blocks is cut.  Plain C++ that reads nothing but knob values and counts -- no device call, no Engine -- so that the
// C ABI's probes (svdf_window_rule, svdf_window_rule_as_cut, svdf_window_block_cuts) and tests/test_window_rule.py run it without a GPU.  The
// routes of svdf_wseq.cpp and svdf_multi.cpp gather the counts and call in here; tests/window_rule.py is the one Python statement of it.
#ifndef SVDF_WSEQ_RULE_H_
#define SVDF_WSEQ_RULE_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "svdf_types.h"

namespace svdf {

// the knobs the rule reads (Engine::wseq_knobs fills them from the knobs of the same names, include/svdfeature_amd.h)
struct WseqKnobs {
    int per_target = 24, per_target_max = 128, per_target_fb = 16, per_target_shared = 12, per_target_child = 3;
    long window = 0;            // amd:window rows, 0 = unset
    bool count_actual = true;   // window_count_actual
    double max_ratio() const { return (double)per_target / (double)per_target_max; }
    bool actual_on() const { return count_actual && window == 0; }
};
// a lane of ordered sub-steps for one side's hot rows: sub-steps of `sub`, at most `cap` updates of a row per window; sub == 0: the side has no lane
struct WseqLane {
    int sub = 0, cap = 0;
};

// How many updates of its own target an entry meets per pass: sum c^2 / sum c (the MEAN over entries, what the calibrations at the uniform
// BASELINE sizes bound at 24 per window) -- and, for skewed data, the MAX: a row that collects far more updates in one window than the
// mean (a Zipf-popular item: 800 where the mean is 24) has all of them computed against its window-start value and overshoots; the pass
// diverges (NaN on Zipf(0.7) items, round 5).  max c is therefore bounded at `per_max` per window, expressed here on the mean's scale.
static inline double mean_updates_met(const std::vector<long> &cnt, double per_mean_over_per_max) {
    double s1 = 0.0, s2 = 0.0;
    long mx = 0;
    for (long c : cnt) { s1 += (double)c; s2 += (double)c * (double)c; mx = std::max(mx, c); }
    return std::max(s1 > 0.0 ? s2 / s1 : 0.0, (double)mx * per_mean_over_per_max);
}
// the term of a class of rows with a per-target mean of its own (`per`: window_per_target_shared, window_per_target_child) under the common cap
// (window_per_target_max), expressed on the item term's scale
static inline double wseq_class_term(const WseqKnobs &K, const std::vector<long> &cnt, int per) {
    return cnt.empty() ? 0.0 : mean_updates_met(cnt, (double)per / (double)K.per_target_max) * (double)K.per_target / (double)per;
}

// OPT-IN and NOT the reference's semantics: the pass is cut into windows; inside a window the shared rows are read as of its start and
// move once, at its end (the N-rank step run by one rank -- the result does not depend on the number of ranks).
// Accuracy contract |dRMSE| <= 1e-4 against the sequential pass, like every N > 1 line; the exact level-scheduled pass stays the default.
// updates_per_target: {item rows, global biases[, feedback rows (instance-sized mass)]}.  Calibrated at the full BASELINE configs[3] sizes
// on three data seeds, 4 and 10 passes (profiles/r04_wstep_calibration.txt): item rows / global biases at 24 per window, feedback rows at 16
// keep |dRMSE| <= 6.2e-5 (SVD++: 24 -> 9.2e-5, 48 -> 1.6e-4; neighbourhood: 64 -> 2.1e-5, 256 -> 1.8e-4 after 10 passes).
static inline long wseq_windows(const WseqKnobs &K, long n, const std::vector<double> &updates_per_target) {
    if (n <= 0) return 1;
    if (K.window > 0) return std::max<long>(1, (n + K.window - 1) / K.window);
    double worst = 0.0;
    for (size_t j = 0; j < updates_per_target.size(); j++)
        worst = std::max(worst, updates_per_target[j] / (double)(j == 2 ? K.per_target_fb : K.per_target));
    return std::max<long>(1, (long)std::ceil(worst));
}

// The window count one side's rows ask for when hot ones move in ordered sub-steps of `sub`.  What the round-5 rule bounded through ONE number
// per row -- updates met per window -- are two different things:
//   * how many changes of a row are computed against one value of it (overshoot: diverges on Zipf items): with sub-steps at most `sub` for every
//     row, so per class -- plain rows at per_plain (window_per_target_shared / window_per_target), side-table children at per_child
//     (window_per_target_child) -- the MEAN over entries  sum_j min(c_j / W, sub) c_j / sum_j c_j  is kept at the class value;
//   * how stale everybody else's view of a hot row gets (they read it as of the window start): no row of the side meets more than `cap` updates
//     per window (window_hot_max 2 048: CPU simulation on a 10 M-rating Zipf(0.7) stream, tools/substep_sim.py: 500 per window +1.5e-5, 1 000
//     +2.8e-5, 2 000 +6.0e-5, 4 000 +9.1e-5 against the 1e-4 contract; on the MI355X at the configs[1] size, 3 data seeds: 1 024 -> max 4.2e-5,
//     2 048 -> 6.6e-5, 3 072 -> 7.2e-5, profiles/r06_hot_lane_calibration.txt).
// The search: from the lower bound ceil(max c / cap), doubling while a class is over its value, then bisection.
static inline long wseq_windows_shared(long n, const std::vector<long> &plain, const std::vector<long> &child, int sub, int cap, int per_plain, int per_child) {
    if (n <= 0) return 1;
    long mx = 0;
    for (long c : plain) mx = std::max(mx, c);
    for (long c : child) mx = std::max(mx, c);
    auto met = [&](const std::vector<long> &cnt, long W) {
        double s = 0.0, s1 = 0.0;
        for (long c : cnt) { s += std::min((double)c / (double)W, (double)sub) * (double)c; s1 += (double)c; }
        return s1 > 0.0 ? s / s1 : 0.0;
    };
    auto ok = [&](long W) { return met(plain, W) <= (double)per_plain && met(child, W) <= (double)per_child; };
    long lo = std::max<long>(1, (mx + cap - 1) / cap);
    if (ok(lo)) return lo;
    long hi = lo;
    while (!ok(hi) && hi < n) hi *= 2;
    while (lo + 1 < hi) { const long mid = (lo + hi) / 2; if (ok(mid)) hi = mid; else lo = mid; }
    return hi;
}

// How often a pass updates every shared target, for the rules of the csr and block sequences: item rows (ci; a feature_item child's row too,
// marked in ichild), global biases (cg) and shared user rows (cs, by id - amd:shared_user_from; a feature_user child marked in uchild).  The
// marks are empty without the table.
struct WseqCounts {
    std::vector<long> ci, cg, cs;
    std::vector<unsigned char> ichild, uchild;
};

// ---- the per-pass rule, one function per route: counts in, W out

// instances given as columns (ratings, rank pairs -- whose items count both entries -- and rank pairs drawn on the device): the item rows'
// term; with a lane (window_hot_sub / window_pair_sub and their caps) the search over one class of rows at window_per_target, the mean over
// ENTRIES (sum_i c_i: n for ratings, 2 n for rank pairs).  amd:window overrides.
static inline long wseq_rule_columns(const WseqKnobs &K, long n, const std::vector<long> &item_count, WseqLane lane) {
    if (lane.sub > 0 && n > 0 && K.window == 0) return wseq_windows_shared(n, item_count, {}, lane.sub, lane.cap, K.per_target, 0);
    return wseq_windows(K, n, {mean_updates_met(item_count, K.max_ratio())});
}

// rows (wseq_from_csr): item rows, global biases, shared user rows and side-table children
static inline long wseq_rule_csr(const WseqKnobs &K, long n, const WseqCounts &C, WseqLane shared_lane, WseqLane item_lane) {
    std::vector<long> ci = C.ci, cs = C.cs;
    // side-table children: a row that is a child anywhere -- a feature_user child among the shared user rows, a feature_item
    // child among the item rows -- is a target of its own kind, with all its updates (as a plain entry too), at window_per_target_child
    std::vector<long> cc, ccu;   // (ccu: the feature_user children alone, for the rule with ordered sub-steps below)
    for (size_t i = 0; i < C.ichild.size(); i++) if (C.ichild[i]) { cc.push_back(ci[i]); ci[i] = 0; }
    for (size_t j = 0; j < C.uchild.size(); j++) if (C.uchild[j]) { cc.push_back(cs[j]); ccu.push_back(cs[j]); cs[j] = 0; }
    // shared user rows are shared targets like item rows: the same rule (mean and most updates met per window), with a per-target mean of their
    // own (window_per_target_shared, 12: a bucket row met by 1/64 of all rows is far hotter than the items the 24 was calibrated on, and 24 left
    // |dRMSE| at 1.3e-4 on the SURVEY 8(d2) variant) and the common cap (window_per_target_max).  Expressed on the item term's scale.
    const double shared_met = wseq_class_term(K, cs, K.per_target_shared), child_met = wseq_class_term(K, cc, K.per_target_child);
    if (shared_lane.sub == 0 && item_lane.sub == 0)
        return wseq_windows(K, n, {std::max({mean_updates_met(ci, K.max_ratio()), shared_met, child_met}), mean_updates_met(C.cg, K.max_ratio())});
    // ordered sub-steps (DESIGN.md sections 6k / 6m): a side whose hot rows ride a lane leaves the common term -- its rows follow
    // wseq_windows_shared -- and the other side keeps its own: item rows at window_per_target, shared user rows at window_per_target_shared,
    // either side's children at window_per_target_child.  The global biases keep their term.
    cc.resize(cc.size() - ccu.size());   // (cc: the feature_item children alone from here on)
    const double item_term = item_lane.sub > 0 ? 0.0 : std::max(mean_updates_met(ci, K.max_ratio()), wseq_class_term(K, cc, K.per_target_child));
    // (a user side that stays in the common term keeps the children's term as it was: the mean over the children of BOTH sides)
    const double user_term = shared_lane.sub > 0 ? 0.0 : std::max(shared_met, ccu.empty() ? 0.0 : child_met);
    long W = wseq_windows(K, n, {std::max(item_term, user_term), mean_updates_met(C.cg, K.max_ratio())});
    if (K.window == 0 && shared_lane.sub > 0) W = std::max(W, wseq_windows_shared(n, cs, ccu, shared_lane.sub, shared_lane.cap, K.per_target_shared, K.per_target_child));
    if (K.window == 0 && item_lane.sub > 0) W = std::max(W, wseq_windows_shared(n, ci, cc, item_lane.sub, item_lane.cap, K.per_target, K.per_target_child));
    return W;
}

// user-group blocks (wseq_from_blocks; user-group trainers load no side tables: no children).  fb_mass: per feedback row, the instance-sized
// updates a pass pushes into it (a feedback row moves by whole-block steps; the caller's loop) -- kept at window_per_target_fb by the same
// measure sum m^2 / sum m.  The lanes (window_block_sub, window_block_item_sub; DESIGN.md sections 6q / 6u) follow the rule of sections 6k / 6m:
// the side's term leaves the common call, its rows follow wseq_windows_shared; amd:window overrides, and the count stays capped by the
// number of blocks.
static inline long wseq_rule_blocks(const WseqKnobs &K, long n, long num_block, const WseqCounts &C, const std::vector<double> &fb_mass, WseqLane shared_lane,
                                    WseqLane item_lane) {
    const double shared_met = wseq_class_term(K, C.cs, K.per_target_shared);   // the shared user rows' term, exactly wseq_rule_csr's
    double m1 = 0.0, m2 = 0.0;
    for (double m : fb_mass) { m1 += m; m2 += m * m; }
    long Wn = wseq_windows(K, n, {item_lane.sub > 0 ? 0.0 : mean_updates_met(C.ci, K.max_ratio()), mean_updates_met(C.cg, K.max_ratio()), m1 > 0.0 ? m2 / m1 : 0.0,
                                  shared_lane.sub > 0 ? 0.0 : shared_met});
    if (shared_lane.sub > 0 && K.window == 0) Wn = std::max(Wn, wseq_windows_shared(n, C.cs, {}, shared_lane.sub, shared_lane.cap, K.per_target_shared, 0));
    if (item_lane.sub > 0 && K.window == 0) Wn = std::max(Wn, wseq_windows_shared(n, C.ci, {}, item_lane.sub, item_lane.cap, K.per_target, 0));
    return std::min<long>(std::max<long>(num_block, 1), Wn);
}

// cuts in blocks (the rule of multi_gpu.block_window_bounds): even block positions moved forward to the next position where no START..END span
// is open.  W + 1 positions, the first 0 and the last num_block.
static inline std::vector<long> wseq_block_cuts(long num_block, const int *extend_tag, long W) {
    std::vector<long> cut{0};
    for (long w = 1; w < W; w++) {
        long pos = std::max<long>(num_block * w / W, cut.back());
        while (pos < num_block && pos > 0 && (extend_tag[pos - 1] == TAG_START || extend_tag[pos - 1] == TAG_MIDDLE)) pos++;
        cut.push_back(pos);
    }
    cut.push_back(num_block);
    return cut;
}

// The automatic window of an amd:gpus handle assumes every item is updated equally often (per_item x num_item instances per window).  A
// resident data set knows better: an instance meets  sum_i c_i^2 / n  updates of its own items per pass (c_i = rows that carry item i), which
// is n / num_item for a uniform catalogue and larger for a skewed one -- THAT is kept at `per_item` per window.  stage_window: the handle's
// rows per window (amd:window, or its automatic value).
static inline long multi_windows_for(const WseqKnobs &K, int gpus, long stage_window, long n, const std::vector<long> &item_count, bool minibatch) {
    long W = std::max<long>(1, (n + stage_window - 1) / stage_window);
    if (K.window > 0 || n <= 0) return W;
    double s2 = 0.0;
    long mx = 0;
    for (long c : item_count) { s2 += (double)c * (double)c; mx = std::max(mx, c); }
    const double per_item = !minibatch ? (gpus <= 2 ? 64.0 : (gpus <= 4 ? 42.0 : 32.0)) : 24.0;
    // ... and no row more than window_per_target_max updates per window (skewed data: mean_updates_met)
    const double need = std::max(s2 / (double)n / per_item, (double)mx / (double)K.per_target_max);
    return std::max<long>(W, (long)std::ceil(need));
}

// ---- the rule on the windows AS CUT
// The per-pass rules above take a row's c updates as spread evenly over the W windows.  The windows are cut at equal positions n w / W, so on a
// file sorted by item, or one that arrives in bursts, they are not: one window can hold all of an item's ratings (window_per_target_max 128
// against 450 met, NaN at the sizes of profiles/r17_window_orders.md).  Knob window_count_actual (default 1): after the per-pass search the rule's
// two quantities are counted on the windows as they are cut, and W is raised until both hold.  A class of shared rows keeps: the mean over its
// entries of min(count of the entry's row in its window, sub) (sub 0: the count) at `target`, and the most updates of one row in one window at
// `cap`.  target <= 0 / cap <= 0: not checked.  Both are taken times kWseqSlack: on a file in random order the actual mean sits above the per-pass
// figure by about 1 (the Poisson term of E[c^2] / E[c]) and the actual maximum above mx / W by sampling noise, and the window counts of the
// calibrations (every one of them on shuffled files) must stay what they are.  amd:window overrides everything.
static constexpr double kWseqSlack = 1.5;
static constexpr int kWseqRounds = 40;
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
// one class whose entries are id columns of the rows (one column for ratings, two for rank pairs)
static inline long wseq_windows_actual_columns(long W, long n, const WseqClass &k, const std::vector<const unsigned *> &cols, double slack, int rounds, bool last_resort) {
    return wseq_windows_actual(W, n, {k}, slack, rounds, last_resort, [&](long b0, long b1, WseqCounter &C) {
        for (const unsigned *c : cols)
            for (long r = b0; r < b1; r++) C.add(0, c[r]);
    });
}

// the item rows of instances given as columns, as the per-pass rule bounds them: window_per_target, and the lane's cap or window_per_target_max
static inline WseqClass wseq_class_columns(const WseqKnobs &K, long num_item, WseqLane lane) {
    return WseqClass{num_item, (double)K.per_target, lane.sub > 0 ? (long)lane.cap : (long)K.per_target_max, lane.sub};
}
static inline long wseq_actual_columns(const WseqKnobs &K, long W, long n, long num_item, const std::vector<const unsigned *> &cols, WseqLane lane) {
    if (!K.actual_on()) return W;
    return wseq_windows_actual_columns(W, n, wseq_class_columns(K, num_item, lane), cols, kWseqSlack, kWseqRounds, true);
}

// the same for rows (wseq_from_csr): item rows, global biases, shared user rows and the side-table children, each class with the target and the cap
// the per-pass rule gives it.  Without a lane the children of both sides are one class (wseq_rule_csr: cc), with one they follow their side.
// What the caller's scan adds its rows' entries to:
class WseqCsrEntries {
 public:
    enum { ITEM = 0, GLOBAL = 1, SHARED = 2, ICHILD = 3, UCHILD = 4 };
    WseqCsrEntries(WseqCounter &counter, const WseqCounts &C0, long num_item, bool lanes) : C(counter), C0(C0), NI(num_item), lanes(lanes) {}
    void global(unsigned g) { C.add(GLOBAL, g); }
    void item(unsigned i) { C.add(!C0.ichild.empty() && C0.ichild[i] ? ICHILD : ITEM, i); }   // (a feature_item child's row: by its own id too)
    void shared(unsigned j) {   // j: id - amd:shared_user_from
        if (!C0.uchild.empty() && C0.uchild[j]) { if (lanes) C.add(UCHILD, j); else C.add(ICHILD, (unsigned)NI + j); }
        else C.add(SHARED, j);
    }
 private:
    WseqCounter &C;
    const WseqCounts &C0;
    const long NI;
    const bool lanes;
};
// scan(b0, b1, entries) adds the entries of the file rows [b0, b1); C0: the marks are what is read (and the number of shared rows)
template <typename Scan>
long wseq_actual_csr(const WseqKnobs &K, long W, long n, const WseqCounts &C0, WseqLane shared_lane, WseqLane item_lane, Scan scan) {
    if (!K.actual_on()) return W;
    const long NI = (long)C0.ci.size(), NS = (long)C0.cs.size();
    const bool lanes = shared_lane.sub > 0 || item_lane.sub > 0;
    const int icap = item_lane.sub > 0 ? item_lane.cap : K.per_target_max, ucap = shared_lane.sub > 0 ? shared_lane.cap : K.per_target_max;
    // (without a lane: UCHILD is unused, the feature_user children count into ICHILD at ids NI + j)
    const std::vector<WseqClass> classes{
        {NI, (double)K.per_target, icap, item_lane.sub},
        {(long)C0.cg.size(), (double)K.per_target, K.per_target_max, 0},
        {NS, (double)K.per_target_shared, ucap, shared_lane.sub},
        {NI + (lanes ? 0 : NS), (double)K.per_target_child, icap, item_lane.sub},
        {lanes ? NS : 0, (double)K.per_target_child, ucap, shared_lane.sub}};
    return wseq_windows_actual(W, n, classes, kWseqSlack, kWseqRounds, true, [&](long b0, long b1, WseqCounter &C) {
        WseqCsrEntries E(C, C0, NI, lanes);
        scan(b0, b1, E);
    });
}

}  // namespace svdf
#endif

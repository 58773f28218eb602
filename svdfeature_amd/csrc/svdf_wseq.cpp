// svdf_wseq.cpp -- one GPU, `amd:step = minibatch`: a pass as a sequence of windows (DESIGN.md sections 6g .. 6v).  The five routes that build
// one -- ratings, rank pairs, rank pairs in HBM, rows, user-group blocks -- gather their counts, ask the window rule (svdf_wseq_rule.h) for the
// number of windows and cut; the windows themselves are built by svdf_window.cpp (plain instances) and svdf_wunit.cpp (user units).
// wseq_train runs a pass over such a sequence.
#include <algorithm>
#include <memory>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>

#include "svdf_engine.h"
#include "svdf_kernels.h"
#include "svdf_internal.h"

namespace svdf {

WseqKnobs Engine::wseq_knobs() const {
    WseqKnobs K;
    K.per_target = wseq_per_target_; K.per_target_max = wseq_per_target_max_; K.per_target_fb = wseq_per_target_fb_;
    K.per_target_shared = wseq_per_target_shared_; K.per_target_child = wseq_per_target_child_;
    K.window = window_set_ ? stage_window_ : 0;
    K.count_actual = wseq_count_actual_ != 0;
    return K;
}

// The windows of a sequence share nothing but the caller's read-only columns: their host builds run on several threads (a quarter of the
// host's hardware threads, at most 32 and at most `wseq_build_threads`), a batch of windows at a time; uploads stay with the calling thread,
// in window order.  A failure inside a worker is reported by the calling thread (the error text is thread-local).
template <typename BuildFn, typename AdoptFn>
static void wseq_build_windows(long W, int max_threads, BuildFn build, AdoptFn adopt_window, int64_t &ns_host, int64_t &ns_adopt) {
    const long hw = (long)std::thread::hardware_concurrency();
    const long T = std::max<long>(1, std::min<long>(std::min<long>(W, max_threads), std::max<long>(1, std::min<long>(32, hw / 4))));
    for (long w0 = 0; w0 < W; w0 += T) {
        const long nb = std::min<long>(T, W - w0);
        std::vector<WUnitHost> H((size_t)nb);
        std::vector<std::string> err((size_t)nb);
        std::vector<char> failed((size_t)nb, 0);
        auto work = [&](long j) {
            try { build(w0 + j, H[(size_t)j]); }
            catch (const std::exception &e) { failed[(size_t)j] = 1; err[(size_t)j] = e.what(); }
        };
        std::unique_ptr<ScopedNs> timer(new ScopedNs(ns_host));   // wall time of the batch's host builds ...
        if (nb == 1) work(0);
        else {
            std::vector<std::thread> th;
            for (long j = 1; j < nb; j++) th.emplace_back(work, j);
            work(0);
            for (auto &t : th) t.join();
        }
        timer.reset();
        for (long j = 0; j < nb; j++) if (failed[(size_t)j]) fail(err[(size_t)j]);
        ScopedNs adopt_timer(ns_adopt);                            // ... and of its windows' allocations, uploads and synchronisations
        for (long j = 0; j < nb; j++) { adopt_window(w0 + j, H[(size_t)j]); H[(size_t)j] = WUnitHost(); }
    }
}

// the counts of the rows [r0, r1) for the rules of the csr and block sequences (WseqCounts, svdf_wseq_rule.h)
void Engine::wseq_count_targets(WseqCounts &C, long r0, long r1, const int64_t *row_ptr, const unsigned *feat_index) const {
    std::vector<long> &ci = C.ci, &cg = C.cg, &cs = C.cs;
    ci.assign((size_t)mp_.num_item, 0); cg.assign((size_t)mp_.num_global, 0);
    cs.assign(shared_user() ? (size_t)std::max<long>(mp_.num_user - (long)shared_user_from_, 0) : 0, 0);
    C.ichild.assign(feat_item_.num_row() ? (size_t)mp_.num_item : 0, 0);
    C.uchild.assign(feat_user_.num_row() ? cs.size() : 0, 0);
    const SideTable &FU = feat_user_, &FI = feat_item_;
    for (long r = r0; r < r1; r++) {
        for (int64_t j = row_ptr[3 * r]; j < row_ptr[3 * r + 1]; j++) { if (feat_index[j] >= (unsigned)mp_.num_global) fail("global feature index exceed setting"); cg[feat_index[j]]++; }
        for (int64_t j = row_ptr[3 * r + 2]; j < row_ptr[3 * r + 3]; j++) {
            const unsigned i = feat_index[j];
            if (i >= (unsigned)mp_.num_item) fail("item feature index exceed bound");
            ci[i]++;
            if (i < FI.num_row()) for (unsigned c = FI.row_ptr[i]; c < FI.row_ptr[i + 1]; c++) { ci[FI.index[c]]++; C.ichild[FI.index[c]] = 1; }
        }
        if (!cs.empty())
            for (int64_t j = row_ptr[3 * r + 1]; j < row_ptr[3 * r + 2]; j++) {
                const unsigned u = feat_index[j];
                if (u >= shared_user_from_ && u < (unsigned)mp_.num_user) cs[u - shared_user_from_]++;
                if (u < FU.num_row())
                    for (unsigned c = FU.row_ptr[u]; c < FU.row_ptr[u + 1]; c++)
                        if (FU.index[c] >= shared_user_from_) { cs[FU.index[c] - shared_user_from_]++; C.uchild[FU.index[c] - shared_user_from_] = 1; }
            }
    }
}
// one built window joins its sequence: uploaded, its first source row recorded
void Engine::wseq_adopt_window(Dataset *ds, const WUnitHost &H, long first) {
    std::unique_ptr<Dataset> c(new Dataset());
    adopt(c.get());
    wunit_adopt(c.get(), H);
    ds->algorithmic_bytes += c->algorithmic_bytes; ds->num_units += c->num_units;
    ds->wchild.push_back(c.release());
    ds->wfirst.push_back(first);
}

Dataset *Engine::wseq_from_csr(long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value) {
    wunit_check_config("dataset_from_csr", true);
    validate_csr_pointers(n, row_ptr);
    WseqCounts C;
    wseq_count_targets(C, 0, n, row_ptr, feat_index);
    const int shared_sub = shared_user() ? wseq_shared_sub_ : 0;
    const int item_sub = wseq_item_sub_;
    const WseqKnobs K = wseq_knobs();
    const WseqLane shared_lane{shared_sub, wseq_shared_max_}, item_lane{item_sub, wseq_item_max_};
    long W = wseq_rule_csr(K, n, C, shared_lane, item_lane);
    const SideTable &FU = feat_user_, &FI = feat_item_;
    const unsigned B = shared_user_from_;
    W = wseq_actual_csr(K, W, n, C, shared_lane, item_lane, [&](long b0, long b1, WseqCsrEntries &E) {
        for (long r = b0; r < b1; r++) {
            for (int64_t j = row_ptr[3 * r]; j < row_ptr[3 * r + 1]; j++) E.global(feat_index[j]);
            for (int64_t j = row_ptr[3 * r + 2]; j < row_ptr[3 * r + 3]; j++) {
                const unsigned i = feat_index[j];
                E.item(i);
                if (i < FI.num_row()) for (unsigned c = FI.row_ptr[i]; c < FI.row_ptr[i + 1]; c++) E.item(FI.index[c]);
            }
            if (!C.cs.empty())
                for (int64_t j = row_ptr[3 * r + 1]; j < row_ptr[3 * r + 2]; j++) {
                    const unsigned u = feat_index[j];
                    if (u >= B && u < (unsigned)mp_.num_user) E.shared(u - B);
                    if (u < FU.num_row())
                        for (unsigned c = FU.row_ptr[u]; c < FU.row_ptr[u + 1]; c++) if (FU.index[c] >= B) E.shared(FU.index[c] - B);
                }
        }
    });
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get()); ds->kind = 8; ds->num_row = n;
    ds->wseq_shared_sub = shared_sub;
    ds->wseq_item_sub = item_sub;
    const bool inplace = wunit_inplace_ != 0;   // a window is summed in place right after its walk (wseq_train): single contributions need no slot
    wseq_build_windows(W, wseq_build_threads_,
        [&](long w, WUnitHost &H) {
            const long b0 = n * w / W, b1 = n * (w + 1) / W;
            wunit_host_from_csr(H, inplace, b1 - b0, row_label + b0, row_ptr + 3 * b0, feat_index, feat_value, true, shared_sub, item_sub);
        },
        [&](long w, const WUnitHost &H) { wseq_adopt_window(ds.get(), H, n * w / W); }, ns_wseq_host_, ns_wseq_adopt_);
    ds->sched.level_ptr = {0, n};
    ds->sched.max_level_size = W > 0 ? (n + W - 1) / W : n;
    return ds.release();
}

Dataset *Engine::wseq_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                  const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                  const float *feat_value) {
    wunit_check_config("dataset_from_blocks");
    validate_block_pointers(num_block, fb_ptr, block_row_ptr);
    validate_csr_pointers((long)(block_row_ptr[num_block] - block_row_ptr[0]), row_ptr + 3 * block_row_ptr[0]);
    const long n = (long)(block_row_ptr[num_block] - block_row_ptr[0]);
    WseqCounts C;   // (user-group trainers load no side tables: no children; cs: the shared user rows of DESIGN.md section 6p)
    wseq_count_targets(C, (long)block_row_ptr[0], (long)block_row_ptr[num_block], row_ptr, feat_index);
    // a feedback row moves by whole-block steps: a block of n rows pushes about n |value| instance-sized updates into every row of its
    // list at once (update_ufeedback, apex_svd_base.h:539-554) -- the same measure as svdf_multi.cpp's window heuristic
    std::vector<double> mass((size_t)std::max(num_fb_rows(), 1), 0.0);
    {
        long open_rows = 0;
        for (long b = 0; b < num_block; b++) {
            const int tag = extend_tag[b];
            if (tag == TAG_DEFAULT || tag == TAG_START) open_rows = 0;
            open_rows += (long)(block_row_ptr[b + 1] - block_row_ptr[b]);
            if (tag == TAG_DEFAULT || tag == TAG_END)
                for (int64_t j = fb_ptr[b]; j < fb_ptr[b + 1]; j++) {
                    if (fb_index[j] >= (unsigned)num_fb_rows()) fail("ufeedback id exceed bound");
                    mass[fb_index[j]] += (double)open_rows * std::fabs((double)fb_value[j]);
                }
        }
    }
    // the lanes of hot shared user rows (knob window_block_sub) and of hot item rows (window_block_item_sub, section 6u)
    const int bsub = block_sub(), isub = block_item_sub();
    const long W0 = wseq_rule_blocks(wseq_knobs(), n, num_block, C, mass, WseqLane{bsub, wseq_block_max_}, WseqLane{isub, wseq_block_item_max_});
    const std::vector<long> cut = wseq_block_cuts(num_block, extend_tag, W0);
    if (num_block > 0 && (extend_tag[num_block - 1] == TAG_START || extend_tag[num_block - 1] == TAG_MIDDLE)) fail("dataset_from_blocks: the last user's END block is missing");
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get()); ds->kind = 8; ds->num_row = n;
    ds->wseq_block_sub = bsub;
    ds->wseq_block_item_sub = isub;
    const bool inplace = wunit_inplace_ != 0;
    wseq_build_windows((long)cut.size() - 1, wseq_build_threads_,
        [&](long w, WUnitHost &H) {
            wunit_host_from_blocks(H, inplace, cut[(size_t)w], cut[(size_t)w + 1], extend_tag, fb_ptr, fb_index, fb_value, block_row_ptr, row_label, row_ptr,
                                   feat_index, feat_value, shared_user(), bsub, isub);
        },
        [&](long w, const WUnitHost &H) { wseq_adopt_window(ds.get(), H, (long)(block_row_ptr[cut[(size_t)w]] - block_row_ptr[0])); },
        ns_wseq_host_, ns_wseq_adopt_);
    ds->sched.level_ptr = {0, n};
    ds->sched.max_level_size = n;
    return ds.release();
}

// Ordered sub-steps (svdf_k_window.hip: k_window_apply): plain ratings of the configurations the window kernels walk with unit values and fp32
// contribution rows, on the one-GPU sequence (in-place sums).
bool Engine::wseq_hot_ok() const {
    return wseq_hot_sub_ > 0 && !contrib_bf16_ && !user_group() && window_rows_allowed() && gpus_ == 1 && !multi_ && !is_peer_;
}
// how often a pass updates every item: the instances' one (item1 == nullptr) or two item columns
std::vector<long> Engine::wseq_item_counts(long n, const unsigned *item, const unsigned *item1) const {
    std::vector<long> ci((size_t)mp_.num_item, 0);
    for (long r = 0; r < n; r++) {
        if (item[r] >= (unsigned)mp_.num_item || (item1 && item1[r] >= (unsigned)mp_.num_item)) fail("item feature index exceed bound");
        ci[item[r]]++;
        if (item1) ci[item1[r]]++;
    }
    return ci;
}
// The window sequence of instances given as columns, cut into windows of equal length: ratings (item, label) or rank pairs (item = the +1 item,
// item1 = the -1 item, no label).  The window count: the per-pass rule on the item counts, then raised on the windows as cut (svdf_wseq_rule.h).
// lane.sub > 0: the windows that hold an item with more than that many slots (both entries of a pair count) are marked for the lane of ordered
// sub-steps (k_window_apply / k_window_apply_pairs).
Dataset *Engine::wseq_from_columns(long n, const unsigned *user, const unsigned *item, const unsigned *item1, const float *label,
                                   const std::vector<long> &item_count, WseqLane lane) {
    const WseqKnobs K = wseq_knobs();
    const int sub = lane.sub;
    long W = wseq_rule_columns(K, n, item_count, lane);
    W = wseq_actual_columns(K, W, n, mp_.num_item, item1 ? std::vector<const unsigned *>{item, item1} : std::vector<const unsigned *>{item}, lane);
    std::vector<char> whot((size_t)W, 0);
    if (sub > 0) {   // one scan with per-item stamps
        std::vector<int> stamp((size_t)mp_.num_item, -1), cnt((size_t)mp_.num_item, 0);
        for (long w = 0; w < W; w++) {
            const long b0 = n * w / W, b1 = n * (w + 1) / W;
            for (long r = b0; r < b1 && !whot[(size_t)w]; r++)
                for (int e = 0; e < (item1 ? 2 : 1); e++) {
                    const unsigned it = e == 0 ? item[r] : item1[r];
                    if (stamp[it] != (int)w) { stamp[it] = (int)w; cnt[it] = 0; }
                    if (++cnt[it] > sub) whot[(size_t)w] = 1;
                }
        }
    }
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get()); ds->kind = 8; ds->num_row = n;
    if (item1) ds->wseq_pair_sub = sub;   // (a sequence of pairs records its window_pair_sub, 0 included: wseq_train)
    // the columns go to HBM in ONE copy each (large pageable copies run at the PCIe rate, 56 GB/s; window-sized ones at a fifth of it), the
    // windows are regrouped from slices of them (svdf_k_wbuild.hip)
    DevBuf<unsigned> d_user, d_item, d_item1;
    DevBuf<float> d_label;
    const bool resident = device_window_ready() && n > 0;
    if (resident) {
        need_device("dataset");
        d_user.upload(user, (size_t)n, stream_); d_item.upload(item, (size_t)n, stream_);
        if (label) d_label.upload(label, (size_t)n, stream_);
        if (item1) d_item1.upload(item1, (size_t)n, stream_);
    }
    for (long w = 0; w < W; w++) {
        const long b0 = n * w / W, b1 = n * (w + 1) / W;
        std::unique_ptr<Dataset> c(new Dataset());
        adopt(c.get());
        if (resident && b1 > b0) {
            window_build_header(c.get(), b1 - b0, item1 != nullptr);
            window_build_resident(c.get(), b1 - b0, d_user.p + b0, d_item.p + b0, label ? d_label.p + b0 : nullptr, item1 ? d_item1.p + b0 : nullptr);
        } else window_build(c.get(), b1 - b0, user + b0, item + b0, label ? label + b0 : nullptr, item1 ? item1 + b0 : nullptr);
        c->win_hot = whot[(size_t)w] != 0;
        ds->algorithmic_bytes += c->algorithmic_bytes; ds->num_units += c->num_units;
        ds->wchild.push_back(c.release());
        ds->wfirst.push_back(b0);
    }
    ds->sched.level_ptr = {0, n};
    ds->sched.max_level_size = W > 0 ? (n + W - 1) / W : n;
    return ds.release();
}

Dataset *Engine::wseq_from_triples(long n, const unsigned *user, const unsigned *item, const float *label) {
    const std::vector<long> ci = wseq_item_counts(n, item, nullptr);
    const bool hot_lane = wseq_hot_ok();   // the lane of hot items: window_hot_sub, window_hot_max
    Dataset *ds = wseq_from_columns(n, user, item, nullptr, label, ci, hot_lane ? WseqLane{wseq_hot_sub_, wseq_hot_max_} : WseqLane{});
    ds->wseq_hot_sub = hot_lane ? wseq_hot_sub_ : 0;   // (the lane's sub-step as it took effect, 0 without the lane: wseq_train)
    return ds;
}

// rank pairs (BASELINE configs[4]): two signed item entries per instance, two contribution slots per pair.  The window rule counts both
// entries; amd:window (pairs per window) overrides -- the demo-rate calibration allows ~320 updates per item per window
// (profiles/r04_pairs_windows_demo_rate.txt), an order of magnitude more than the rating default kept here.
// window_pair_sub > 0 (ordered sub-steps for hot items of rank pairs): fp32 slots, random-order trainers, the one-GPU sequence
void Engine::wseq_pair_check(const char *what) const {
    wseq_sub_check(what, "window_pair_sub", "ordered sub-steps for hot items of rank pairs", "dataset_window_from_pairs",
                   "the N-rank exchange sums every slot on the wire", true);
    check(gpus_ == 1 && !multi_ && !is_peer_,
          "window data sets: window_pair_sub > 0 (ordered sub-steps for hot items of rank pairs) is for the one-GPU window sequence; amd:gpus > 1 sums every slot on the wire");
    check(wunit_width_ok(), "window data sets: window_pair_sub > 0 needs num_factor <= 256 (the lane of rank pairs has no wide rows)");
}
Dataset *Engine::wseq_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg) {
    const std::vector<long> ci = wseq_item_counts(n, pos, neg);
    const int psub = wseq_pair_sub_;
    if (psub > 0) wseq_pair_check("dataset_from_pairs");
    // ordered sub-steps for hot items: the lane of wseq_from_triples with the pair knobs
    return wseq_from_columns(n, user, pos, neg, nullptr, ci, psub > 0 ? WseqLane{psub, wseq_pair_max_} : WseqLane{});
}
// The same sequence for a pass of rank pairs that is in HBM already (the device sampler's columns, file order: Engine::rank_pass_device; DESIGN.md
// section 6v).  What wseq_from_pairs reads from host arrays -- the item counts, the per-pass W, its raise on the windows as cut -- comes from
// svdf_k_rankwin.hip: only the num_item counts and two integers per search round cross PCIe.  Without the lane of ordered sub-steps (the caller
// keeps window_pair_sub > 0 off this route).  The windows are regrouped from slices of the columns like wseq_from_columns' resident form.
Dataset *Engine::wseq_from_device_pairs(long n, const unsigned *d_user, const unsigned *d_i0, const float *d_v0, const unsigned *d_i1) {
    const long NI = mp_.num_item, E = 2 * n;
    std::vector<long> ci((size_t)NI, 0);
    std::unique_ptr<ScopedNs> timer(new ScopedNs(ns_rank_rule_));
    DevBuf<unsigned> d_pos, d_neg, d_cnt, d_state, k0, k1, v0, v1;
    const WseqKnobs K = wseq_knobs();
    const bool actual = K.actual_on() && n > 0;
    const bool merged = d_v0 != nullptr;   // (else the columns are pos / neg already)
    if (n > 0) {
        need_device("dataset");
        if (merged) { d_pos.reserve((size_t)n); d_neg.reserve((size_t)n); }
        d_cnt.reserve((size_t)std::max<long>(NI, 1)); d_state.reserve(4);
        if (actual) { k0.reserve((size_t)E); k1.reserve((size_t)E); v0.reserve((size_t)E); v1.reserve((size_t)E); }
        HIPCHECK(hipMemsetAsync(d_cnt.p, 0, (size_t)std::max<long>(NI, 1) * sizeof(unsigned), stream_));
        HIPCHECK(hipMemsetAsync(d_state.p, 0, 4 * sizeof(unsigned), stream_));
        if (merged)
            launch_rank_window_columns(n, d_user, d_i0, d_v0, d_i1, mp_.num_user, NI, d_pos.p, d_neg.p, actual ? k0.p : nullptr, actual ? v0.p : nullptr, d_cnt.p, d_state.p,
                                       stream_);
        else launch_rank_window_pairs(n, d_user, d_i0, d_i1, mp_.num_user, NI, actual ? k0.p : nullptr, actual ? v0.p : nullptr, d_cnt.p, d_state.p, stream_);
        std::vector<unsigned> hc((size_t)NI);
        unsigned hs[4] = {0u, 0u, 0u, 0u};
        if (NI > 0) HIPCHECK(hipMemcpyAsync(hc.data(), d_cnt.p, (size_t)NI * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(hs, d_state.p, sizeof(hs), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        HIPCHECK(hipGetLastError());
        if (hs[0] != 0u) return nullptr;
        for (long i = 0; i < NI; i++) ci[(size_t)i] = (long)hc[(size_t)i];
    }
    long W = wseq_rule_columns(K, n, ci, WseqLane{});
    if (actual) {
        try {
            DevBuf<char> tmp;
            const size_t tb = rank_window_sort_bytes(E);
            tmp.reserve(std::max<size_t>(tb, 1));
            rank_window_sort(tmp.p, tb, k0.p, k1.p, v0.p, v1.p, E, NI, stream_);
            DevBuf<unsigned long long> d_out;
            d_out.reserve(2);
            W = wseq_windows_actual_counted(W, n, wseq_class_columns(K, NI, WseqLane{}), E, kWseqSlack, kWseqRounds, true,
                                            [&](long w, unsigned long long &sum, unsigned long long &worst) {
                                                rank_window_sums(k1.p, v1.p, E, n, w, d_out.p, &sum, &worst, stream_);
                                            });
        } catch (const std::runtime_error &e) {
            fail(e.what());
        }
        k0.release(); k1.release(); v0.release(); v1.release();
    }
    timer.reset(new ScopedNs(ns_rank_wbuild_));
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get()); ds->kind = 8; ds->num_row = n;
    ds->wseq_pair_sub = 0;
    const unsigned *w_pos = merged ? d_pos.p : d_i0, *w_neg = merged ? d_neg.p : d_i1;
    for (long w = 0; w < W; w++) {
        const long b0 = n * w / W, b1 = n * (w + 1) / W;
        std::unique_ptr<Dataset> c(new Dataset());
        adopt(c.get());
        window_build_header(c.get(), b1 - b0, true, true);
        if (b1 > b0) window_build_resident(c.get(), b1 - b0, d_user + b0, w_pos + b0, nullptr, w_neg + b0);   // (returns after the window's read-back: the columns outlive every read)
        else {   // a pass that drew no pair: one window without instances, the arrays of window_build at n = 0
            need_device("dataset");
            c->win_urec.reserve(1); c->item.reserve(1); c->win_slot.reserve(1); c->win_item1.reserve(1); c->win_slot1.reserve(1); c->ival.reserve(1); c->win_ival1.reserve(1);
            c->win_iptr.reserve((size_t)NI + 1);
            HIPCHECK(hipMemsetAsync(c->win_iptr.p, 0, ((size_t)NI + 1) * sizeof(int), stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
            c->win_has_pos = window_keeps_positions();
            if (c->win_has_pos) c->win_pos.reserve(1);
            c->sched_signature = schedule_signature();
            c->win_item_lo = NI; c->win_item_hi = -1;
            c->unit_values = true;
            c->num_units = 0;
            c->sched.level_ptr = {0, 0};
            c->sched.max_level_size = 0;
        }
        ds->algorithmic_bytes += c->algorithmic_bytes; ds->num_units += c->num_units;
        ds->wchild.push_back(c.release());
        ds->wfirst.push_back(b0);
    }
    ds->sched.level_ptr = {0, n};
    ds->sched.max_level_size = W > 0 ? (n + W - 1) / W : n;
    return ds.release();
}

// one pass over a window sequence: per window the users' walks, then the per-target sums added in place (two launches per window)
void Engine::wseq_train(Dataset *ds) {
    const DevParams &P = params();
    bool any_hot = false;
    long max_slots = 1;
    for (Dataset *c : ds->wchild) if (c->kind == 5 && c->win_hot) { any_hot = true; max_slots = std::max(max_slots, c->win_slots); }
    const bool pair_seq = ds->wseq_pair_sub >= 0;   // built by wseq_from_pairs: its hot windows belong to the pair lane (window_pair_sub), not to window_hot_sub
    if (pair_seq) {
        check(ds->wseq_pair_sub == wseq_pair_sub_,
              "train_dataset: the window sequence was built with another window_pair_sub (ordered sub-steps for hot items of rank pairs); build the data set again after changing the knob");
        if (wseq_pair_sub_ > 0) wseq_pair_check("train_dataset");
    }
    if (ds->wseq_hot_sub >= 0)   // built by wseq_from_triples: the threshold between cold and hot rows was fixed then (the windows' marks, the window count)
        check(ds->wseq_hot_sub == (wseq_hot_ok() ? wseq_hot_sub_ : 0),
              "train_dataset: the window sequence was built with another window_hot_sub (ordered sub-steps for hot items); build the data set again after changing the knob");
    const bool hot_lane = any_hot && (pair_seq || wseq_hot_ok());
    if (any_hot) check(hot_lane, "train_dataset: the window sequence was built with ordered sub-steps for hot items (window_hot_sub); the configuration changed since");
    if (hot_lane) d_clabel_.reserve((size_t)max_slots);
    if (ds->wseq_shared_sub >= 0)
        check(ds->wseq_shared_sub == (shared_user() ? wseq_shared_sub_ : 0),
              "train_dataset: the window sequence was built with another window_shared_sub (ordered sub-steps for hot shared user rows); build the data set again after changing the knob");
    if (ds->wseq_block_sub >= 0) {
        check(ds->wseq_block_sub == block_sub(),
              "train_dataset: the window sequence was built with another window_block_sub (ordered sub-steps for hot shared user rows of SVD++ blocks); build the data set again after changing the knob");
        check(ds->wseq_block_item_sub == block_item_sub(),
              "train_dataset: the window sequence was built with another window_block_item_sub (ordered sub-steps for hot item rows of SVD++ blocks); build the data set again after changing the knob");
        long most = 0;   // the second record plane: sized once, for the largest window's hot records (of both sides)
        for (Dataset *c : ds->wchild) if (c->wu_feedback && c->wu_nhot + c->wu_nihot > 0) most = std::max(most, c->wu_nhrec);
        if (most > 0) { d_hfb_.reserve((size_t)most * (size_t)pitch_); d_hfbb_.reserve((size_t)most); }
    }
    if (ds->wseq_item_sub >= 0)
        check(ds->wseq_item_sub == wseq_item_sub_,
              "train_dataset: the window sequence was built with another window_item_sub (ordered sub-steps for hot item rows); build the data set again after changing the knob");
    for (Dataset *c : ds->wchild) {
        if (c->kind == 5) {
            d_contrib_.reserve((size_t)std::max<long>(c->win_slots, 1) * (size_t)pitch_);
            d_cbias_.reserve((size_t)std::max<long>(c->win_slots, 1));
            WindowSchedule S = window_view(c);
            if (hot_lane && c->win_hot) { S.hot_sub = pair_seq ? wseq_pair_sub_ : wseq_hot_sub_; S.clabel = d_clabel_.p; }
            launch_window_users(P, S, window_slots_, window_groups_, stream_);
            if (S.hot_sub > 0 && pair_seq) {   // walk, hot apply (does not write the model: a pair reads its OTHER item's row), then hot rows moved in + the cold sums
                launch_window_apply_pairs(P, S, mp_.num_item, stream_);
                launch_window_pair_sums(S, pitch_, mp_.num_factor, mp_.num_item, dW_.p + (size_t)item_off_ * pitch_, dbias_.p + item_off_, stream_);
                n_launches_++;
            } else if (S.hot_sub > 0) launch_window_apply(P, S, mp_.num_item, dW_.p + (size_t)item_off_ * pitch_, dbias_.p + item_off_, stream_);
            else launch_window_items_local(S, pitch_, mp_.num_factor, 0, mp_.num_item, dW_.p + (size_t)item_off_ * pitch_, dbias_.p + item_off_, stream_, c->win_slots);
        } else {
            wunit_train(c);
            // hot shared user rows in ordered sub-steps: after the walk (its records) and before the sums (which move the finished rows in); the
            // workgroups run one hot row each, so the launch lasts as long as the hottest row's chain of sub-steps
            if (c->wu_nhot > 0) {
                launch_wunit_apply_shared(P, wunit_view(c), stream_, c->wu_feedback);   // (user-group windows: the FB build, knob window_block_sub -- section 6q)
                n_launches_++;
                if (c->wu_feedback) n_block_hot_ += c->wu_nhot;   // counter 35
            }
            if (c->wu_nihot > 0) {   // hot item rows likewise (neither launch writes the model; user-group windows: the FB build, knob window_block_item_sub -- section 6u)
                launch_wunit_apply_item(P, wunit_view(c), c->wu_nihot, stream_, c->wu_feedback);
                n_launches_++;
                if (c->wu_feedback) n_block_item_hot_ += c->wu_nihot;   // counter 36
            }
            wunit_sum(c, nullptr, 0);
        }
        n_launches_ += 2;
        window_trained_ = nullptr;
    }
}

}  // namespace svdf

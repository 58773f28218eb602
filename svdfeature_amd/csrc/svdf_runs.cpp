// svdf_runs.cpp -- host side of the runs schedule (svdf_k_runs.hip; knob "runs_exec"): plain (user, item, rating)
// triples of the contract configuration become runs of up to R consecutive ratings of one item, formed and level-scheduled in HBM.
// Nothing of SVDFeature::update_inner (apex_svd_base.h:456-462) changes: same instances, every row's touches in file order, the item's row
// kept in registers across a run instead of being written and read back between two of its ratings.
#include <algorithm>
#include <array>
#include <vector>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "svdf_engine.h"
#include "svdf_kernels.h"
#include "svdf_internal.h"

namespace svdf {

bool Engine::runs_config_ok() const {
    return runs_exec_ != 0 && !host_only_ && device_sched_ && !user_group() && basic_fast_path_allowed() && mtype_.extend_type == 0 && mtype_.active_type == ACT_LINEAR &&
           tp_.reg_method == 0 && mp_.user_nonnegative == 0 && mp_.no_user_bias == 0 && u_param_.bound.empty() && i_param_.bound.empty() && (mp_.num_factor == 64 || mp_.num_factor == 128) &&
           basic_i8_ != 0 && store_mode_ == 0;
}

// The in-level sort key (R - length) * NI + item takes values up to R * NI - 1, and the scheduler's key column holds 32 bits
static constexpr bool runs_order_key_fits(int R, unsigned NI) { return (uint64_t)R * (uint64_t)NI <= 0xFFFFFFFFull; }
static_assert(runs_order_key_fits(7, 1u << 27) && runs_order_key_fits(7, 613566756u) && !runs_order_key_fits(7, 613566757u), "R = 7: 7 * NI up to 2^32 - 1");
static_assert(runs_order_key_fits(4, (1u << 30) - 1u) && !runs_order_key_fits(4, 1u << 30), "R = 4: NI below 2^30");
static_assert(runs_order_key_fits(2, (1u << 31) - 1u) && !runs_order_key_fits(2, 1u << 31), "R = 2: NI below 2^31");

// What the order costs the pass, counted once over the level-sorted columns for either order (svdf_dataset_info 11 / 12; SVDF_VERBOSE)
void Engine::runs_order_stats(Dataset *ds) {
    const long nunit = ds->num_units;
    const size_t nlev = ds->sched.num_levels();
    if (nunit <= 0 || nlev == 0 || nlev >= 0x7FFFFFFFul) return;
    DevBuf<long> lp;
    DevBuf<unsigned long long> tot;
    lp.upload(ds->sched.level_ptr.data(), nlev + 1, stream_);
    tot.reserve(9);
    HIPCHECK(hipMemsetAsync(tot.p, 0, 9 * sizeof(unsigned long long), stream_));
    RunSchedule S;
    memset(&S, 0, sizeof(S));
    for (int j = 0; j < ds->rn_len; j++) S.user[j] = ds->rn_user[j].p;
    launch_runs_order_stats(S, lp.p, (int)nlev, nunit, ds->rn_len, mp_.num_factor == 128 ? 4 : 8, tot.p, stream_);
    HIPCHECK(hipGetLastError());
    unsigned long long h[9];
    HIPCHECK(hipMemcpyAsync(h, tot.p, sizeof(h), hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));
    ds->rn_wave_steps = (int64_t)h[0];
    ds->rn_mixed_sets = (int64_t)h[1];
    for (int c = 1; c < 8; c++) ds->rn_hist[c] = (int64_t)h[1 + c];
}

// nullptr: the configuration has no runs kernel: the caller builds the plain level schedule
Dataset *Engine::runs_dataset_from_triples(long n, const unsigned *user, const unsigned *item, const float *label) {
    if (!runs_config_ok() || n < runs_min_rows_ || n >= 0x7FFFFFF0L) return nullptr;
    const int RF = std::max(2, std::min(7, runs_len_));           // ratings per run at most (the level scheduler takes 8 row slots per unit: 1 item + 7 users)
    const int R = RF <= 2 ? 2 : (RF <= 4 ? 4 : 7);               // the kernel's width: columns beyond a run's length hold SLOT_ABSENT
    const unsigned NU = (unsigned)mp_.num_user, NI = (unsigned)mp_.num_item;
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get());
    ds->kind = 10; ds->num_row = n; ds->rn_len = R;
    // the raw columns stay in file order: the evaluator and predict_dataset score them as they are
    ds->user.upload(user, (size_t)n, stream_);
    ds->item.upload(item, (size_t)n, stream_);
    ds->label.upload(label, (size_t)n, stream_);
    ds->unit_values = true;
    DevBuf<unsigned> flag, ka, kb, va, vb, prev, head, head_of, unit_at, c_item, c_user;
    DevBuf<unsigned char> idx;
    DevBuf<float> c_label;
    flag.reserve(4);
    HIPCHECK(hipMemsetAsync(flag.p, 0, 4 * sizeof(unsigned), stream_));
    launch_runs_check(ds->user.p, ds->item.p, n, NU, NI, flag.p, stream_);
    unsigned hflag = 0;
    HIPCHECK(hipMemcpyAsync(&hflag, flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));
    if (hflag & 1u) fail("user feature index exceed bound");
    if (hflag & 2u) fail("item feature index exceed bound");
    ka.reserve((size_t)n); kb.reserve((size_t)n); va.reserve((size_t)n); vb.reserve((size_t)n);
    prev.reserve((size_t)n); head.reserve((size_t)n); head_of.reserve((size_t)n); unit_at.reserve((size_t)n); idx.reserve((size_t)n);
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    struct FreeTmp { void *&p; ~FreeTmp() { if (p) (void)hipFree(p); } } free_tmp{tmp};
    // 1. the previous rating of every rating's user
    HIPCHECK(hipMemcpyAsync(ka.p, ds->user.p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToDevice, stream_));
    launch_runs_iota(va.p, n, stream_);
    device_sort_pairs_u32(ka.p, kb.p, va.p, vb.p, n, &tmp, &tmp_bytes, stream_);
    launch_runs_prev(kb.p, vb.p, n, prev.p, stream_);
    // 2. the item-major list, 3. runs
    HIPCHECK(hipMemcpyAsync(ka.p, ds->item.p, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToDevice, stream_));
    launch_runs_iota(va.p, n, stream_);
    device_sort_pairs_u32(ka.p, kb.p, va.p, vb.p, n, &tmp, &tmp_bytes, stream_);
    launch_runs_form(kb.p, vb.p, n, NI, prev.p, RF, head.p, head_of.p, idx.p, stream_);
    // 4. runs numbered by the file position of their head
    const long nunit = device_exclusive_scan_u32(head.p, unit_at.p, n, &tmp, &tmp_bytes, stream_);
    HIPCHECK(hipGetLastError());
    // 5. the runs' columns
    c_item.reserve((size_t)nunit); c_user.reserve((size_t)R * (size_t)nunit); c_label.reserve((size_t)R * (size_t)nunit);
    launch_runs_fill_u32(c_user.p, (long)R * nunit, (unsigned)SLOT_ABSENT, stream_);
    HIPCHECK(hipMemsetAsync(c_label.p, 0, (size_t)R * (size_t)nunit * sizeof(float), stream_));
    launch_runs_fill(ds->user.p, ds->item.p, ds->label.p, n, unit_at.p, head_of.p, idx.p, nunit, c_item.p, c_user.p, c_label.p, stream_);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(stream_));
    ka.release(); kb.release(); va.release(); vb.release(); prev.release(); head.release(); head_of.release(); unit_at.release(); idx.release();
    // 6. the level schedule of the runs: slot 0 the item row, slots 1 .. R the user rows (absent ones skipped by the scheduler)
    const unsigned *res[SVDF_SCHED_MAX_SLOTS];
    unsigned off[SVDF_SCHED_MAX_SLOTS], limit[SVDF_SCHED_MAX_SLOTS];
    const char *msg[SVDF_SCHED_MAX_SLOTS];
    res[0] = c_item.p; off[0] = NU; limit[0] = NI; msg[0] = "item feature index exceed bound";
    std::vector<DUCol> du{DUCol{c_item.p, &ds->rn_item}};
    std::vector<DFCol> df;
    for (int j = 0; j < R; j++) {
        res[1 + j] = c_user.p + (size_t)j * (size_t)nunit; off[1 + j] = 0u; limit[1 + j] = NU; msg[1 + j] = "user feature index exceed bound";
        du.push_back(DUCol{c_user.p + (size_t)j * (size_t)nunit, &ds->rn_user[j]});
        df.push_back(DFCol{c_label.p + (size_t)j * (size_t)nunit, &ds->rn_label[j]});
    }
    // the order inside a level (knob "runs_order", with sort_batches = 1): by (R - length) * NI + item, or by item.  The key's largest value R * NI - 1 has
    // to fit the scheduler's 32-bit key column (it widens the sort to 64 bits by itself when level bits + key bits need it); beyond that: item order
    const unsigned *sort_key = sort_batches_ == 1 ? c_item.p : nullptr;
    unsigned sort_max = NI;
    DevBuf<unsigned> c_key;
    if (sort_batches_ == 1 && runs_order_ == 1 && runs_order_key_fits(R, NI)) {
        c_key.reserve((size_t)nunit);
        launch_runs_order_key(c_item.p, c_user.p, nunit, R, NI, c_key.p, stream_);
        HIPCHECK(hipGetLastError());
        sort_key = c_key.p; sort_max = (unsigned)R * NI;
        ds->rn_order = 1;
    }
    if (ds->rn_order == 1) {
        // the sorted order without the columns, a level's row sets dealt into the XCDs' eight shares (k_runs_order_deal), then the columns in that order
        schedule_device_columns(ds.get(), nunit, 1 + R, res, off, limit, msg, sort_key, sort_max, {}, {});
        const size_t nlev = ds->sched.num_levels();
        if (nlev > 0 && nlev < 0x7FFFFFFFul) {
            DevBuf<long> lp;
            DevBuf<int> dealt;
            lp.upload(ds->sched.level_ptr.data(), nlev + 1, stream_);
            dealt.reserve((size_t)nunit);
            launch_runs_order_deal(ds->order_dev.p, dealt.p, lp.p, (int)nlev, nunit, mp_.num_factor == 128 ? 4 : 8, stream_);
            HIPCHECK(hipMemcpyAsync(ds->order_dev.p, dealt.p, (size_t)nunit * sizeof(int), hipMemcpyDeviceToDevice, stream_));
            HIPCHECK(hipGetLastError());
            HIPCHECK(hipStreamSynchronize(stream_));
        }
        for (const DUCol &c : du) { c.dst->reserve((size_t)nunit); device_gather_u32(c.src, ds->order_dev.p, c.dst->p, nunit, stream_); }
        for (const DFCol &c : df) { c.dst->reserve((size_t)nunit); device_gather_f32(c.src, ds->order_dev.p, c.dst->p, nunit, stream_); }
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream_));
    } else {
        schedule_device_columns(ds.get(), nunit, 1 + R, res, off, limit, msg, sort_key, sort_max, du, df);
    }
    ds->num_units = nunit;
    runs_order_stats(ds.get());
    ds->algorithmic_bytes = n * (8L * mp_.num_factor * 2 + 8 * 2 + 16 + 8 * 2);
    if (runs_stage_) runs_stage_build(ds.get());
    return ds.release();
}

// Operand staging (knob "runs_stage"): (1 + R) * nunit slots of one row + one bias, the dst word of each, the first slot of every
// row, and the labels once more in the slots' order.  Slot s * (1 + R) + j = operand j of the run at position s of the level order (run-major: what one
// wave needs of the dst words, biases and labels is contiguous; the rows stay plane-major, row j * nunit + s).  Built once per data set from the level-sorted columns and the schedule's order; refused -- the data set then keeps reading and writing W, the
// same bits -- when the slots do not fit 31 bits, half of the free device memory or the knob "runs_stage_max_mb", or when the allocation fails.
namespace {
template <typename T>
bool try_reserve(DevBuf<T> &b, size_t n) {   // DevBuf::reserve without the failure: false, the error cleared
    b.release();
    if (hipMalloc((void **)&b.p, (n ? n : 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
    b.cap = n ? n : 1;
    return true;
}
}  // namespace
void Engine::runs_stage_build(Dataset *ds) {
    ds->rn_stage_state = 2;
    ds->rn_stage_bytes = 0;
    const long nunit = ds->num_units, nrow = (long)mp_.num_user + (long)mp_.num_item;
    const int R = ds->rn_len;
    const long m = (long)(1 + R) * nunit;
    if (nunit <= 0) return;
    const int64_t bytes = (int64_t)m * ((int64_t)pitch_ * 4 + 8) + (int64_t)R * nunit * 4 + (int64_t)nrow * 4;   // rows, biases + dst words, labels, first[]
    auto refuse = [&](const char *why) {
        ds->rn_stage_row.release(); ds->rn_stage_bias.release(); ds->rn_dst.release(); ds->rn_first.release(); ds->rn_label_rm.release();
        if (!getenv("SVDF_QUIET"))
            fprintf(stderr, "[svdfeature_amd] data set of %ld rows: no operand staging (%.1f MB: %s); its runs keep reading and writing W\n", (long)ds->num_row, (double)bytes / 1048576.0, why);
    };
    if (item_off_ != user_off_ + (unsigned)mp_.num_user || n_uiset_ >= 0x7FFFFFFFL) { refuse("W_user and W_item are not adjacent in W"); return; }
    if (m >= 0x7FFFFFFFL) { refuse("more than 2^31 slots"); return; }
    if (runs_stage_max_mb_ >= 0 && bytes > (int64_t)runs_stage_max_mb_ * 1048576) { refuse("above runs_stage_max_mb"); return; }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); refuse("hipMemGetInfo failed"); return; }
    if ((uint64_t)bytes > (uint64_t)free_b / 2) { refuse("more than half of the free device memory"); return; }
    if (!try_reserve(ds->rn_stage_row, (size_t)m * (size_t)pitch_) || !try_reserve(ds->rn_stage_bias, (size_t)m) || !try_reserve(ds->rn_dst, (size_t)m) ||
        !try_reserve(ds->rn_first, (size_t)nrow) || !try_reserve(ds->rn_label_rm, (size_t)R * (size_t)nunit)) { refuse("hipMalloc failed"); return; }
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    struct FreeTmp { void *&p; ~FreeTmp() { if (p) (void)hipFree(p); } } free_tmp{tmp};
    try {
        DevBuf<unsigned> pos_of, ka, kb, va, vb;   // scratch of the build: 16 bytes per slot
        if (!try_reserve(pos_of, (size_t)nunit) || !try_reserve(ka, (size_t)m) || !try_reserve(kb, (size_t)m) || !try_reserve(va, (size_t)m) || !try_reserve(vb, (size_t)m)) {
            refuse("hipMalloc failed");
            return;
        }
        RunSchedule S;
        memset(&S, 0, sizeof(S));
        S.item = ds->rn_item.p;
        for (int j = 0; j < R; j++) { S.user[j] = ds->rn_user[j].p; S.label[j] = ds->rn_label[j].p; }
        launch_runs_stage_links(S, ds->order_dev.p, nunit, R, (unsigned)mp_.num_user, user_off_, pos_of.p, ka.p, kb.p, va.p, vb.p, &tmp, &tmp_bytes, ds->rn_dst.p,
                                ds->rn_first.p, nrow, stream_);
        launch_runs_label_rm(S, nunit, R, ds->rn_label_rm.p, stream_);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(stream_));
    } catch (const std::exception &ex) {
        (void)hipGetLastError();
        refuse(ex.what());
        return;
    }
    ds->rn_stage_state = 1;
    ds->rn_stage_row0 = user_off_;
    ds->rn_stage_bytes = bytes;
}

#ifdef SVDF_RUNS_STAMPS
// Timing build only (the Makefile never sets SVDF_RUNS_STAMPS; profiles/r39_runs_store.md, part 0).  With SVDF_RUNS_STAMPS=<pass number, from 1> in the environment that
// staged pass of the engine runs with clock stamps: lane 0 of every wave writes wall_clock64() at 0 entry, 1 slot words + item row here, 2 .. 4 user rows
// 0 .. 2 here (where the gather waits for them one by one), 5 every row here, 6 last store issued.  Reduced per launch over the waves that had work and
// printed; SVDF_RUNS_STAMPS_OUT=<file> also gets one line per launch.  -> true: the pass's launches are done
bool Engine::runs_probe_pass(Dataset *ds, const DevParams &P, RunSchedule &S) {
    const char *e = getenv("SVDF_RUNS_STAMPS");
    if (!e || !S.dst || n_runs_passes_ + 1 != (int64_t)atol(e)) return false;
    const Schedule &sc = ds->sched;
    const size_t nlev = sc.num_levels();
    const int G = runs_sets_ >= 2 ? 2 : 1, wpb = runs_block_ / 64, per_wave = P.k == 128 ? 4 : 8;
    std::vector<long> w0(nlev + 1, 0);
    for (size_t l = 0; l < nlev; l++) {
        const long per_block = (long)wpb * G * per_wave;
        long grid = (sc.level_ptr[l + 1] - sc.level_ptr[l] + per_block - 1) / per_block;
        if (P.xcd_remap) grid = (grid + 7) & ~7L;
        w0[l + 1] = w0[l] + grid * wpb;
    }
    DevBuf<unsigned long long> buf;
    buf.reserve((size_t)w0[nlev] * 8);
    HIPCHECK(hipMemsetAsync(buf.p, 0, (size_t)w0[nlev] * 64, stream_));
    S.stamps = buf.p;
    for (size_t l = 0; l < nlev; l++) {
        S.stamp_wave0 = w0[l];
        launch_basicmf_runs_soa(P, S, sc.level_ptr[l], sc.level_ptr[l + 1], ds->rn_len, runs_sets_, runs_block_, stream_);
    }
    HIPCHECK(hipGetLastError());
    std::vector<unsigned long long> h((size_t)w0[nlev] * 8);
    HIPCHECK(hipMemcpyAsync(h.data(), buf.p, h.size() * 8, hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));
    S.stamps = nullptr;
    int dev = 0, khz = 100000;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
    const double us = 1000.0 / (double)khz;
    FILE *out = getenv("SVDF_RUNS_STAMPS_OUT") ? fopen(getenv("SVDF_RUNS_STAMPS_OUT"), "w") : nullptr;
    if (out) fprintf(out, "launch,waves,ramp_us,span_us,gap_after_us,head_us,gather_us,steps_us,row0_us,row1_us,row2_us,rest_us\n");
    enum { NC = 10 };
    std::vector<double> col[NC];   // over the launches of at least 4000 live waves
    unsigned long long prev_last = 0;
    std::vector<double> rowv[NC];
    std::vector<std::array<double, NC>> rows(nlev);
    for (size_t l = 0; l < nlev; l++) {
        unsigned long long emin = ~0ull, emax = 0, smax = 0;
        double sum[7] = {0, 0, 0, 0, 0, 0, 0};
        long cnt[7] = {0, 0, 0, 0, 0, 0, 0}, live = 0;
        for (long w = w0[l]; w < w0[l + 1]; w++) {
            const unsigned long long *t = &h[(size_t)w * 8];
            if (!t[6]) continue;
            live++;
            emin = std::min(emin, t[0]); emax = std::max(emax, t[0]); smax = std::max(smax, t[6]);
            sum[0] += (double)(t[1] - t[0]); sum[1] += (double)(t[5] - t[1]); sum[2] += (double)(t[6] - t[5]);
            unsigned long long at = t[1];
            for (int r = 0; r < 3; r++)
                if (t[2 + r]) { sum[3 + r] += (double)(t[2 + r] - at); cnt[3 + r]++; at = t[2 + r]; }
            sum[6] += (double)(t[5] - at);
        }
        std::array<double, NC> v{};
        if (live) {
            v[0] = (double)(emax - emin) * us; v[1] = (double)(smax - emin) * us;
            for (int c = 0; c < 3; c++) v[3 + c] = sum[c] / (double)live * us;
            for (int r = 0; r < 3; r++) v[6 + r] = cnt[3 + r] ? sum[3 + r] / (double)cnt[3 + r] * us : 0.0;
            v[9] = sum[6] / (double)live * us;
            if (l > 0 && prev_last) rows[l - 1][2] = ((double)emin - (double)prev_last) * us;   // the gap BEHIND the previous launch
        }
        rows[l] = v;
        rows[l][2] = 0.0;
        prev_last = live ? smax : 0;
        rowv[0].push_back((double)live);
    }
    for (size_t l = 0; l < nlev; l++) {
        if (out) { fprintf(out, "%zu,%.0f", l, rowv[0][l]); for (int c = 0; c < NC; c++) fprintf(out, ",%.3f", rows[l][c]); fprintf(out, "\n"); }
        if (rowv[0][l] >= 4000.0 && l + 1 < nlev)
            for (int c = 0; c < NC; c++) col[c].push_back(rows[l][c]);
    }
    if (out) fclose(out);
    static const char *names[NC] = {"entry ramp (first to last wave's entry)", "span (first entry to last store issued)", "gap to the next launch's first entry", "head: slot words + item row", "gather of the user rows", "steps and stores", "user row 0", "user row 1", "user row 2", "the rest of the gather"};
    fprintf(stderr, "[svdfeature_amd] runs stamps, pass %s, runs_store %d: %zu launches, %zu of them with >= 4000 live waves; over those, microseconds (mean / median):\n", e, runs_store_, nlev, col[0].size());
    for (int c = 0; c < NC; c++) {
        std::vector<double> &x = col[c];
        if (x.empty()) continue;
        double m = 0.0;
        for (double y : x) m += y;
        std::sort(x.begin(), x.end());
        fprintf(stderr, "[svdfeature_amd]   %-44s %8.3f / %8.3f\n", names[c], m / (double)x.size(), x[x.size() / 2]);
    }
    return true;
}
#endif

void Engine::runs_train(Dataset *ds) {
    const DevParams &P = params();
    RunSchedule S;
    memset(&S, 0, sizeof(S));
    S.item = ds->rn_item.p;
    for (int j = 0; j < ds->rn_len; j++) { S.user[j] = ds->rn_user[j].p; S.label[j] = ds->rn_label[j].p; }
    const Schedule &sc = ds->sched;
    if (runs_stage_ && ds->rn_stage_state == 0) runs_stage_build(ds);   // a data set built while the knob was off
    if (runs_staged(ds)) {
        // W is the truth between passes: every touched row goes to the slot of its first touch, the levels hand it on from slot to slot, its last touch writes it home
        S.dst = ds->rn_dst.p; S.stage_row = ds->rn_stage_row.p; S.stage_bias = ds->rn_stage_bias.p; S.label_rm = ds->rn_label_rm.p; S.nunit = ds->num_units;
        S.store = runs_store_;
        launch_runs_stage_in(P, ds->rn_first.p, (long)mp_.num_user + (long)mp_.num_item, user_off_, S.stage_row, S.stage_bias, 1 + ds->rn_len, ds->num_units, stream_);
        n_launches_++;
    }
#ifdef SVDF_RUNS_STAMPS
    if (!runs_probe_pass(ds, P, S))
#endif
    for (size_t l = 0; l < sc.num_levels(); l++) launch_basicmf_runs_soa(P, S, sc.level_ptr[l], sc.level_ptr[l + 1], ds->rn_len, runs_sets_, runs_block_, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_ += (int64_t)sc.num_levels();
    n_batches_ += (int64_t)sc.num_levels();
    n_runs_passes_++;
}

}  // namespace svdf

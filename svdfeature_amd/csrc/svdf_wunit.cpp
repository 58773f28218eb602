// svdf_wunit.cpp -- host side of the window-minibatch step for user units (svdf_k_wunit.hip): builds the
// window data sets of user-group (SVD++) blocks and of rows with global features -- units, segments, regrouped rows, contribution
// slots in file order --, the shape checks and the config refusals.  The one-GPU window sequence behind `amd:step = minibatch` that is built
// from these windows: svdf_wseq.cpp.
//
// What the step replaces in the reference: the shared-state part of SVDPPFeature::update (apex_svd_base.h:568-582: prepare_ufeedback
// :523-538, update_ufeedback :539-554) and of update_no_decay / regularize on item rows and global biases (:383-427, :188-210) is
// applied at the window's end instead of instance by instance; the private part (the user's row, bias and feedback state) is exact.
#include <algorithm>
#include <memory>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>

#include "svdf_engine.h"
#include "svdf_kernels.h"
#include "svdf_internal.h"

namespace svdf {


namespace {
struct HostSeg {
    unsigned user = 0;
    int64_t fb_begin = 0, fb_count = 0;   // into the caller's feedback arrays
    size_t row_first = 0, row_count = 0;  // into seg_rows (source row ids)
    bool has_user = false;
};
}  // namespace

WUnitSchedule Engine::wunit_view(const Dataset *ds) const {
    WUnitSchedule S;
    S.units = ds->wu_units.p; S.nunits = ds->num_units; S.segs = ds->wu_segs.p;
    S.label = ds->label.p; S.uval = ds->unit_values ? nullptr : ds->uval.p;
    S.rptr = ds->wu_estride > 0 ? nullptr : ds->wu_rptr.p; S.estride = ds->wu_estride;
    S.ent = ds->wu_ent.p; S.fbent = ds->wu_fbent.p;
    S.contrib = d_contrib_.p; S.cbias = d_cbias_.p; S.gcontrib = d_gcontrib_.p;
    S.tptr = ds->wu_tptr.p; S.gptr = ds->wu_gptr.p;
    S.nfb_rows = user_group() ? (long)num_fb_rows() : 0; S.nitem_rows = mp_.num_item; S.nglobal = mp_.num_global;
    S.contrib_bf16 = contrib_bf16_ ? 1 : 0;
    S.fbrec = ds->wu_defer_fb ? ds->wu_fbrec.p : nullptr; S.dvec = d_dvec_.p; S.dbias = d_dbias_.p;
    S.user_bias = mp_.no_user_bias ? 0 : 1;
    S.touched = ds->wu_ntouched >= 0 ? ds->wu_touched.p : nullptr; S.ntouched = std::max<long>(ds->wu_ntouched, 0);
    const bool sh = ds->wu_nshared > 0;
    S.uptr = sh ? ds->wu_uptr.p : nullptr; S.upos = sh ? ds->wu_upos.p : nullptr; S.uent = sh ? ds->wu_uent.p : nullptr;
    S.nshared_rows = ds->wu_nshared; S.shared_from = sh ? shared_user_from_ : 0u;
    S.iptr = ds->wu_ichild ? ds->wu_iptr.p : nullptr; S.ient = ds->wu_ichild ? ds->wu_ient.p : nullptr;
    const bool hot = ds->wu_nhot + ds->wu_nihot > 0;
    S.hot = hot ? ds->wu_hot.p : nullptr; S.hrec = hot ? ds->wu_hrec.p : nullptr; S.nhot = ds->wu_nhot;
    S.item_sub = ds->wu_feedback ? block_item_sub() : wseq_item_sub_;   // user-group windows: knob window_block_item_sub
    S.hot_sub = ds->wu_feedback ? block_sub() : wseq_shared_sub_;   // user-group windows: knob window_block_sub
    S.hfb = d_hfb_.p; S.hfbb = d_hfbb_.p;
    return S;
}

// user_units: the data set would take the user-unit kernels (svdf_k_wunit.hip, svdf_k_wave.hip) on a route that keeps one lane group per row (num_factor
// <= 256: `auto`, the staged route, the N-rank paths, the rank-buffer route); the windows of plain ratings / rank pairs (svdf_k_window.hip) have wide rows
// and ask with false.  (The one-GPU sequence under amd:step = minibatch has wide user units too: wunit_wide_ok.)
bool Engine::wunit_config_ok(bool user_units) const {
    return trainer_ready_ && mtype_.extend_type == 0 && !relaxed() && !lazy_decay() && mp_.common_latent_space == 0 && feat_user_.num_row() == 0 &&
           feat_item_.num_row() == 0 && g_stride_ == 1 && (!user_units || wunit_width_ok()) && (!user_group() || mp_.common_feedback_space == 0);
}
bool Engine::wunit_width_ok() const { return mp_.num_factor <= 256; }
// the one-GPU sequence of user units (wseq_from_csr / wseq_from_blocks): its general walk, in-place sums and scoring kernels have wide rows, a wave
// per unit / target / row.  Everything else that trains user units asks wunit_width_ok.
bool Engine::wunit_wide_ok() const { return mp_.num_factor <= max_supported_factor(); }
void Engine::wunit_check_config(const char *what, bool tables_ok) const {
    check(trainer_ready_, "dataset: init_trainer has not been called");
    check(mtype_.extend_type == 0, "window data sets: the base solvers only (extend_type 0)");
    if (side_tables()) {   // feature_user / feature_item: the one-GPU window sequence of random-order rows only
        check(!user_group(), "window data sets: feature_user / feature_item side tables are not supported with user-group (SVD++) trainers");
        check(strcmp(what, "dataset_window_from_csr") != 0,
              "svdf_dataset_window_from_csr: feature_user / feature_item side tables are for the one-GPU window sequence (amd:step = minibatch); "
              "the N-rank exchange has no place for their children");
    }
    check(!relaxed() && !lazy_decay() && mp_.common_latent_space == 0 && (tables_ok || !side_tables()) && g_stride_ == 1,
          "window data sets: no side tables, relaxed ids, lazy decay or shared latent space");
    if (side_tables()) {
        check(feat_user_.num_row() == 0 || shared_user(),
              "window data sets: a feature_user side table needs amd:shared_user_from (its children are shared user rows, ids >= B)");
        check(!contrib_bf16_, "window data sets: feature_user / feature_item side tables need amd:contrib = fp32");
    }
    // ordered sub-steps for hot shared user rows and for hot item rows (6m): the one-GPU sequence of random-order rows, fp32 slots
    if (wseq_shared_sub_ > 0)
        wseq_sub_check(what, "window_shared_sub", "ordered sub-steps for hot shared user rows", "dataset_window_from_csr",
                       "the N-rank exchange (amd:gpus > 1) has no place for user rows");
    if (wseq_item_sub_ > 0) {
        wseq_sub_check(what, "window_item_sub", "ordered sub-steps for hot item rows", "dataset_window_from_csr",
                       "the N-rank exchange (amd:gpus > 1) sums every slot on the wire");
        check(wunit_inplace_ != 0, "window data sets: window_item_sub > 0 (ordered sub-steps for hot item rows) needs the in-place sums (knob wunit_inplace = 1)");
    }
    if (block_sub() > 0) wseq_block_check(what);
    if (block_item_sub() > 0) wseq_block_item_check(what);
    // width: the one-GPU sequences (amd:step = minibatch) take wide rows through the general walk; the N-rank builders and the sub-step lanes (one lane
    // group per slot) stay at 256 factors
    const bool sequence = strcmp(what, "dataset_from_csr") == 0 || strcmp(what, "dataset_from_blocks") == 0;
    if (sequence && !wunit_width_ok()) {
        check(wunit_wide_ok(), "window data sets: num_factor <= 1024");
        check(wseq_shared_sub_ == 0, "window data sets: window_shared_sub > 0 (ordered sub-steps for hot shared user rows) needs num_factor <= 256 (the lane has no wide rows)");
        check(wseq_item_sub_ == 0, "window data sets: window_item_sub > 0 (ordered sub-steps for hot item rows) needs num_factor <= 256 (the lane has no wide rows)");
        check(block_sub() == 0, "window data sets: window_block_sub > 0 (ordered sub-steps for hot shared user rows of SVD++ blocks) needs num_factor <= 256 (the lane has no wide rows)");
        check(block_item_sub() == 0, "window data sets: window_block_item_sub > 0 (ordered sub-steps for hot item rows of SVD++ blocks) needs num_factor <= 256 (the lane has no wide rows)");
    } else
        check(wunit_width_ok(), "window data sets: num_factor <= 256");
    check(!user_group() || mp_.common_feedback_space == 0, "window data sets: user-group trainers need a feedback space of their own (common_feedback_space = 0)");
    check(!shared_user() || (shared_user_from_ >= 1 && (long)shared_user_from_ <= (long)mp_.num_user), "amd:shared_user_from must be in 1 .. num_user");
}
// What a sub-step knob that is on refuses, with its cause: bf16 slots, user-group trainers, and the N-rank exchange -- `entry` is the call that step
// builds its windows through, `nrank` says why it cannot serve the lane.  entry_only: the third refusal is about `entry` alone (the caller refuses
// amd:gpus > 1 in words of its own); otherwise it covers amd:gpus > 1 as well.
void Engine::wseq_sub_check(const char *what, const char *knob, const char *desc, const char *entry, const char *nrank, bool entry_only) const {
    auto refuse = [&](bool ok, const std::string &before, const char *after) {
        if (!ok) fail(before + knob + " > 0 (" + desc + ")" + after);
    };
    refuse(!contrib_bf16_, "window data sets: ", " needs amd:contrib = fp32");
    refuse(!user_group(), "window data sets: ", " is not supported with user-group (SVD++) trainers");
    if (strcmp(what, entry) == 0 || !(entry_only || (gpus_ == 1 && !multi_ && !is_peer_)))
        refuse(false, std::string("svdf_") + entry + ": ", (std::string(" is for the one-GPU window sequence (amd:step = minibatch); ") + nrank).c_str());
}

// window_block_sub in effect (user-group trainer under amd:shared_user_from): fp32 slots, the one-GPU window sequence.  (The
// in-place sums are asked for by the builder, once a row is hot.)
void Engine::wseq_block_check(const char *what) const {
    check(!contrib_bf16_, "window data sets: window_block_sub > 0 (ordered sub-steps for hot shared user rows of SVD++ blocks) needs amd:contrib = fp32");
    check(strcmp(what, "dataset_window_from_blocks") != 0 && gpus_ == 1 && !multi_ && !is_peer_,
          "svdf_dataset_window_from_blocks: window_block_sub > 0 (ordered sub-steps for hot shared user rows of SVD++ blocks) is for the one-GPU window sequence "
          "(amd:step = minibatch); the N-rank exchange (amd:gpus > 1) has no place for user rows");
}

// window_block_item_sub in effect (user-group trainer): fp32 slots, the one-GPU window sequence.  (The in-place sums are asked
// for by the builder, once a row is hot.)
void Engine::wseq_block_item_check(const char *what) const {
    check(!contrib_bf16_, "window data sets: window_block_item_sub > 0 (ordered sub-steps for hot item rows of SVD++ blocks) needs amd:contrib = fp32");
    check(strcmp(what, "dataset_window_from_blocks") != 0 && gpus_ == 1 && !multi_ && !is_peer_,
          "svdf_dataset_window_from_blocks: window_block_item_sub > 0 (ordered sub-steps for hot item rows of SVD++ blocks) is for the one-GPU window sequence "
          "(amd:step = minibatch); the N-rank exchange (amd:gpus > 1) sums every slot on the wire");
}

// Common builder.  segs: in FILE order; seg_rows: source row ids (rows of a segment in file order).  by_row_order: random-order
// windows, where the file order of the contributions is the order of the source rows (segments of different users interleave);
// otherwise (user-group passes) a segment's rows are consecutive in the file and its feedback scatter follows them.
void Engine::wunit_build_host(WUnitHost &H, bool inplace, const void *segs_v, size_t nseg, const std::vector<int64_t> &seg_rows, bool by_row_order,
                              long num_src_row, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value,
                              const unsigned *fb_index, const float *fb_value, const int64_t *priv_pos, bool children, int shared_sub, int item_sub) const {
    const HostSeg *segs = static_cast<const HostSeg *>(segs_v);
    const long NU = mp_.num_user, NI = mp_.num_item, NG = mp_.num_global, NF = user_group() ? (long)num_fb_rows() : 0;
    // side-table children (children: the one-GPU window sequence): [c0, c1) of an id into the table's columns
    const SideTable &FU = feat_user_, &FI = feat_item_;
    auto kids = [&](const SideTable &T, unsigned id, unsigned &c0, unsigned &c1) {
        c0 = c1 = 0;
        if (children && id < T.num_row()) { c0 = T.row_ptr[id]; c1 = T.row_ptr[id + 1]; }
        return c1 > c0;
    };
    // shared user rows (priv_pos: the private entry of every source row; the other user entries are ids >= amd:shared_user_from, and so are
    // feature_user children): targets after the item rows, only when the window holds such an entry -- otherwise the window is laid out exactly
    // as without the key.  feature_item children: a child section, only when the window holds one.
    bool has_shared = false, has_ichild = false;
    unsigned c0, c1;
    if (priv_pos)
        for (long r = 0; r < num_src_row && !has_shared; r++) {
            has_shared = row_ptr[3 * r + 2] - row_ptr[3 * r + 1] > 1;
            for (int64_t j = row_ptr[3 * r + 1]; j < row_ptr[3 * r + 2] && !has_shared; j++) has_shared = kids(FU, feat_index[j], c0, c1);
        }
    if (children)
        for (long r = 0; r < num_src_row && !has_ichild; r++)
            for (int64_t j = row_ptr[3 * r + 2]; j < row_ptr[3 * r + 3] && !has_ichild; j++) has_ichild = kids(FI, feat_index[j], c0, c1);
    const unsigned SB = has_shared ? shared_user_from_ : 0u;
    const long NS = has_shared ? NU - (long)SB : 0, NT = NF + NI + NS;
    const bool feedback = user_group();
    H.feedback = feedback;
    // ---- units: the segments of one user, in file order; launch order by cost (rows + feedback entries), descending
    std::vector<int> unit_of_user((size_t)NU, -1);
    std::vector<unsigned> unit_user;
    std::vector<long> unit_cost;
    std::vector<int> seg_unit(nseg, -1);
    std::vector<int> unit_nseg;
    for (size_t s = 0; s < nseg; s++) {
        if (!segs[s].has_user) continue;   // a span without rows: its feedback delta is zero (tmp - old = 0), nothing to do
        const unsigned u = segs[s].user;
        if (unit_of_user[u] < 0) { unit_of_user[u] = (int)unit_user.size(); unit_user.push_back(u); unit_cost.push_back(0); unit_nseg.push_back(0); }
        const int un = unit_of_user[u];
        seg_unit[s] = un;
        unit_cost[(size_t)un] += (long)segs[s].row_count + (long)segs[s].fb_count;
        unit_nseg[(size_t)un]++;
    }
    const size_t nunit = unit_user.size();
    std::vector<int> launch(nunit);
    std::iota(launch.begin(), launch.end(), 0);
    std::stable_sort(launch.begin(), launch.end(), [&](int a, int b) { return unit_cost[(size_t)a] > unit_cost[(size_t)b]; });
    std::vector<int> pos_of_unit(nunit);
    for (size_t j = 0; j < nunit; j++) pos_of_unit[(size_t)launch[j]] = (int)j;
    std::vector<WinUnit> &units = H.units;
    units.assign(nunit, WinUnit{});
    {
        long acc = 0;
        for (size_t j = 0; j < nunit; j++) {
            const int un = launch[j];
            units[j] = WinUnit{unit_user[(size_t)un], (int)acc, 0, 0, WinSeg{0, 0, 0, 0}};
            acc += unit_nseg[(size_t)un];
        }
    }
    // segments in launch order of their unit, file order inside a unit; rows regrouped accordingly
    size_t nseg_used = 0;
    for (size_t s = 0; s < nseg; s++) nseg_used += seg_unit[s] >= 0;
    std::vector<WinSeg> &wsegs = H.wsegs;
    wsegs.assign(nseg_used, WinSeg{});
    std::vector<int> seg_new(nseg, -1);
    for (size_t s = 0; s < nseg; s++) {
        if (seg_unit[s] < 0) continue;
        WinUnit &U = units[(size_t)pos_of_unit[(size_t)seg_unit[s]]];
        seg_new[s] = U.seg_begin + U.seg_count;
        U.seg_count++;
        U.rows += (int)segs[s].row_count;
    }
    long nrow = 0, nfbe = 0;
    for (size_t s = 0; s < nseg; s++) if (seg_unit[s] >= 0) { nrow += (long)segs[s].row_count; nfbe += (long)segs[s].fb_count; }
    check(nrow < (1L << 30) && nfbe < (1L << 30), "window data sets: at most 2^30-1 rows / feedback entries per window");
    // row and feedback ranges of the new segments: walk the segments in NEW order
    std::vector<size_t> seg_by_new(nseg_used);
    for (size_t s = 0; s < nseg; s++) if (seg_new[s] >= 0) seg_by_new[(size_t)seg_new[s]] = s;
    std::vector<long> newrow_of_src((size_t)num_src_row, -1);
    {
        long racc = 0, facc = 0;
        for (size_t q = 0; q < nseg_used; q++) {
            const HostSeg &h = segs[seg_by_new[q]];
            wsegs[q] = WinSeg{(int)facc, (int)h.fb_count, (int)racc, (int)h.row_count};
            for (size_t j = 0; j < h.row_count; j++) newrow_of_src[(size_t)seg_rows[h.row_first + j]] = racc + (long)j;
            racc += (long)h.row_count; facc += h.fb_count;
        }
    }
    // ---- regrouped rows: label, user value, entries = [global entries | item entries]
    std::vector<float> &w_label = H.w_label, &w_uval = H.w_uval;
    w_label.assign((size_t)nrow, 0.0f); w_uval.assign((size_t)nrow, 0.0f);
    std::vector<int> &rptr = H.rptr;
    rptr.assign((size_t)2 * nrow + 1, 0);
    bool unit_uval = true;
    long nent = 0;
    int fixed_ng = -2;   // -2 unknown, -1 not fixed
    std::vector<long> src_of_new((size_t)nrow, -1);
    for (long r = 0; r < num_src_row; r++) if (newrow_of_src[(size_t)r] >= 0) src_of_new[(size_t)newrow_of_src[(size_t)r]] = r;
    H.pos.assign(src_of_new.begin(), src_of_new.end());
    for (long nr = 0; nr < nrow; nr++) {
        const long r = src_of_new[(size_t)nr];
        const int64_t p0 = row_ptr[3 * r], p1 = row_ptr[3 * r + 1], p2 = row_ptr[3 * r + 2], p3 = row_ptr[3 * r + 3];
        const int ng = (int)(p1 - p0), ni = (int)(p3 - p2);
        rptr[(size_t)2 * nr] = (int)nent; rptr[(size_t)2 * nr + 1] = (int)(nent + ng);
        nent += ng + ni;
        check(nent < (1L << 30), "window data sets: at most 2^30-1 feature entries per window");
        if (fixed_ng == -2) fixed_ng = (ni == 1) ? ng : -1;
        else if (fixed_ng >= 0 && !(ni == 1 && ng == fixed_ng)) fixed_ng = -1;
        const int64_t pv = priv_pos ? priv_pos[r] : p1;
        w_label[(size_t)nr] = row_label[r];
        w_uval[(size_t)nr] = feat_value[pv];
        if (feat_value[pv] != 1.0f) unit_uval = false;
        if (has_shared) {   // the row's user entries in entry order, the private one by position
            H.uptr.push_back((int)H.uent.size());
            for (int64_t j = p1; j < p2; j++) {   // each entry followed by its feature_user children (the private one's: the front of [um, u1))
                if (j == pv) H.upos.push_back((int)H.uent.size() - H.uptr.back());
                else H.uent.push_back(WinEnt{feat_index[j] - SB, feat_value[j], 0, 0});
                if (kids(FU, feat_index[j], c0, c1))
                    for (unsigned c = c0; c < c1; c++) H.uent.push_back(WinEnt{FU.index[c] - SB, FU.value[c], 0, 0});
            }
        }
    }
    rptr[(size_t)2 * nrow] = (int)nent;
    if (has_shared) {
        H.uptr.push_back((int)H.uent.size());
        check((long)H.uent.size() < (1L << 30), "window data sets: at most 2^30-1 shared user entries per window");
    }
    std::vector<WinEnt> &ent = H.ent;
    ent.assign((size_t)nent, WinEnt{0u, 0.0f, 0, 0});
    // ---- slots: counts per target, then file-order assignment
    std::vector<int> &tptr = H.tptr, &gptr = H.gptr;
    tptr.assign((size_t)NT + 1, 0); gptr.assign((size_t)NG + 1, 0);
    for (const WinEnt &u : H.uent) tptr[(size_t)(NF + NI + u.idx) + 1]++;
    std::vector<unsigned> seen;   // duplicate check inside a row / a list
    for (long nr = 0; nr < nrow; nr++) {
        const long r = src_of_new[(size_t)nr];
        const int64_t p0 = row_ptr[3 * r], p1 = row_ptr[3 * r + 1], p2 = row_ptr[3 * r + 2], p3 = row_ptr[3 * r + 3];
        int e = rptr[(size_t)2 * nr];
        seen.clear();
        for (int64_t j = p0; j < p1; j++, e++) {
            if (feat_index[j] >= (unsigned)NG) fail("global feature index exceed setting");
            ent[(size_t)e].idx = feat_index[j]; ent[(size_t)e].val = feat_value[j];
            for (unsigned x : seen) if (x == feat_index[j]) fail("window data sets: a global id listed twice in one row");
            seen.push_back(feat_index[j]);
            gptr[(size_t)feat_index[j] + 1]++;
        }
        seen.clear();
        if (has_ichild) H.iptr.push_back((int)H.ient.size());
        for (int64_t j = p2; j < p3; j++, e++) {
            if (feat_index[j] >= (unsigned)NI) fail("item feature index exceed bound");
            ent[(size_t)e].idx = feat_index[j]; ent[(size_t)e].val = feat_value[j];
            for (unsigned x : seen) if (x == feat_index[j]) fail("window data sets: an item id listed twice in one row");
            seen.push_back(feat_index[j]);
            tptr[(size_t)(NF + feat_index[j]) + 1]++;
            if (has_ichild && kids(FI, feat_index[j], c0, c1))   // the entry's feature_item children; pad = the parent's position in ent
                for (unsigned c = c0; c < c1; c++) {
                    H.ient.push_back(WinEnt{FI.index[c], FI.value[c], 0, e});
                    tptr[(size_t)(NF + FI.index[c]) + 1]++;
                }
        }
    }
    if (has_ichild) {
        H.iptr.push_back((int)H.ient.size());
        check((long)H.ient.size() < (1L << 30), "window data sets: at most 2^30-1 feature_item children per window");
    }
    std::vector<WinEnt> &fbent = H.fbent;
    fbent.assign((size_t)nfbe, WinEnt{0u, 0.0f, 0, 0});
    for (size_t q = 0; q < nseg_used; q++) {
        const HostSeg &h = segs[seg_by_new[q]];
        std::vector<unsigned> ids(fb_index + h.fb_begin, fb_index + h.fb_begin + h.fb_count);
        std::sort(ids.begin(), ids.end());
        for (size_t j = 1; j < ids.size(); j++) if (ids[j] == ids[j - 1]) fail("window data sets: a feedback id listed twice in one block");
        for (int64_t j = 0; j < h.fb_count; j++) {
            const unsigned f = fb_index[h.fb_begin + j];
            if (f >= (unsigned)NF) fail("ufeedback id exceed bound");
            fbent[(size_t)wsegs[q].fb_begin + (size_t)j].idx = f; fbent[(size_t)wsegs[q].fb_begin + (size_t)j].val = fb_value[h.fb_begin + j];
            tptr[(size_t)f + 1]++;
        }
    }
    // one-GPU window sequences: a row that meets exactly ONE contribution in this window gets no slot (slot -1): the unit applies it in place
    // with the sum kernel's operations (apply_single, svdf_device.h) -- nobody else reads or writes that row inside the window
    // deferred feedback scatter: every feedback contribution keeps a slot (a record, not a row) -- the sum kernel forms (w + d val) - w itself
    const bool defer_fb = feedback && wunit_defer_fb_ != 0;
    // ordered sub-steps (window_shared_sub): a shared user row with more than shared_sub contributions in this window is hot.
    // A window with a hot row keeps a slot for EVERY contribution: k_wunit_apply_shared re-reads item rows, biases, globals and the other shared
    // rows after the walk, and they must still be what they were at the window start.
    if (shared_sub > 0 && has_shared)
        for (long j = 0; j < NS; j++)
            if (tptr[(size_t)(NF + NI + j) + 1] > shared_sub) H.hot.push_back(WinHot{(int)j, 0, 0, 0});
    H.nhot_user = (long)H.hot.size();
    // the same for the item range (window_item_sub, section 6m): a plain item entry's row, a feature_item child's row, or both -- the slots count
    if (item_sub > 0)
        for (long i = 0; i < NI; i++)
            if (tptr[(size_t)(NF + i) + 1] > item_sub) H.hot.push_back(WinHot{(int)i, 0, 0, 0});
    std::vector<unsigned char> single;
    if (inplace && H.hot.empty()) {
        single.assign((size_t)NT, 0);
        for (size_t t = defer_fb ? (size_t)NF : 0; t < (size_t)NT; t++) if (tptr[t + 1] == 1) { single[t] = 1; tptr[t + 1] = 0; }
    }
    auto take_slot = [&](std::vector<int> &cur, size_t t) { return (!single.empty() && single[t]) ? -1 : cur[t]++; };
    for (size_t t = 0; t < (size_t)NT; t++) tptr[t + 1] += tptr[t];
    for (size_t g = 0; g < (size_t)NG; g++) gptr[g + 1] += gptr[g];
    std::vector<int> tcur(tptr.begin(), tptr.end() - 1), gcur(gptr.begin(), gptr.end() - 1);
    if (defer_fb) H.fbrec.assign((size_t)tptr[(size_t)NF], WinFbRec{0, 0.0f});
    auto row_slots = [&](long nr) {
        const long r = src_of_new[(size_t)nr];
        const int ng = (int)(row_ptr[3 * r + 1] - row_ptr[3 * r]);
        const int e0 = rptr[(size_t)2 * nr], e1 = e0 + ng, e2 = rptr[(size_t)2 * nr + 2];
        for (int e = e0; e < e1; e++) ent[(size_t)e].slot = gcur[ent[(size_t)e].idx]++;
        for (int e = e1; e < e2; e++) ent[(size_t)e].slot = take_slot(tcur, (size_t)NF + ent[(size_t)e].idx);
        if (has_shared)
            for (int e = H.uptr[(size_t)nr]; e < H.uptr[(size_t)nr + 1]; e++) H.uent[(size_t)e].slot = take_slot(tcur, (size_t)(NF + NI) + H.uent[(size_t)e].idx);
        if (has_ichild)
            for (int e = H.iptr[(size_t)nr]; e < H.iptr[(size_t)nr + 1]; e++) H.ient[(size_t)e].slot = take_slot(tcur, (size_t)NF + H.ient[(size_t)e].idx);
    };
    if (by_row_order) {
        for (long r = 0; r < num_src_row; r++) if (newrow_of_src[(size_t)r] >= 0) row_slots(newrow_of_src[(size_t)r]);
    } else {
        for (size_t s = 0; s < nseg; s++) {   // file order of the segments: rows, then the feedback scatter of the segment's end
            if (seg_new[s] < 0) continue;
            const WinSeg &w = wsegs[(size_t)seg_new[s]];
            for (int j = 0; j < w.row_count; j++) row_slots((long)w.row_begin + j);
            for (int j = 0; j < w.fb_count; j++) {
                WinEnt &f = fbent[(size_t)w.fb_begin + (size_t)j];
                f.slot = take_slot(tcur, (size_t)f.idx);
                if (defer_fb) H.fbrec[(size_t)f.slot] = WinFbRec{seg_new[s], f.val};
            }
        }
    }
    if (!H.hot.empty()) {   // the hot rows' slot ranges and records (slots are in file order: the record of a slot is found through its entry)
        check(inplace, H.nhot_user > 0 ? (feedback ? "window data sets: window_block_sub > 0 (ordered sub-steps for hot shared user rows of SVD++ blocks) needs the in-place sums (knob wunit_inplace = 1)"
                                                   : "window data sets: ordered sub-steps for shared user rows need the in-place sums (knob wunit_inplace = 1)")
                                       : feedback ? "window data sets: window_block_item_sub > 0 (ordered sub-steps for hot item rows of SVD++ blocks) needs the in-place sums (knob wunit_inplace = 1)"
                                                  : "window data sets: ordered sub-steps for item rows need the in-place sums (knob wunit_inplace = 1)");
        std::vector<int> hot_of((size_t)(NI + NS), -1);   // by target - NF: item rows, then shared user rows
        int rec = 0;
        for (size_t q = 0; q < H.hot.size(); q++) {
            WinHot &h = H.hot[q];
            const size_t t = (size_t)NF + ((long)q < H.nhot_user ? (size_t)NI : 0) + (size_t)h.j;
            h.b = tptr[t]; h.e = tptr[t + 1]; h.rec = rec;
            rec += h.e - h.b;
            hot_of[t - (size_t)NF] = (int)q;
        }
        H.hrec.assign((size_t)rec, WinHotRec{0, 0});
        auto record = [&](int q, int slot, long nr, int pos) { H.hrec[(size_t)(H.hot[(size_t)q].rec + slot - H.hot[(size_t)q].b)] = WinHotRec{(int)nr, pos}; };
        for (long nr = 0; nr < nrow; nr++) {
            if (H.nhot_user > 0)
                for (int e = H.uptr[(size_t)nr]; e < H.uptr[(size_t)nr + 1]; e++) {
                    WinEnt &u = H.uent[(size_t)e];
                    const int q = hot_of[(size_t)NI + u.idx];
                    if (q < 0) continue;
                    // user-group windows (section 6q): the mark carries the record's index, where the walk leaves the span's feedback state
                    u.pad = feedback ? 1 + H.hot[(size_t)q].rec + u.slot - H.hot[(size_t)q].b : 1;
                    record(q, u.slot, nr, e);
                }
            if ((long)H.hot.size() == H.nhot_user) continue;
            // hot item rows (svdf_types.h, WinHotRec): a plain entry is marked pad = 1 (user-group windows, section 6u: 1 + the record's index, as a hot
            // uent above), position e; a child carries its slot as -2 - slot, position ~c
            for (int e = rptr[(size_t)2 * nr + 1]; e < rptr[(size_t)2 * nr + 2]; e++) {
                WinEnt &it = ent[(size_t)e];
                const int q = hot_of[it.idx];
                if (q < 0) continue;
                it.pad = feedback ? 1 + H.hot[(size_t)q].rec + it.slot - H.hot[(size_t)q].b : 1;
                record(q, it.slot, nr, e);
            }
            if (has_ichild)
                for (int c = H.iptr[(size_t)nr]; c < H.iptr[(size_t)nr + 1]; c++) {
                    WinEnt &ch = H.ient[(size_t)c];
                    const int q = hot_of[ch.idx];
                    if (q < 0) continue;
                    record(q, ch.slot, nr, ~c);
                    ch.slot = -2 - ch.slot;
                }
        }
    }
    if (inplace) {   // the in-place sums visit only the targets that have slots (a window touches a fraction of the rows; singles keep none)
        H.has_touched = true;
        // a hot row's entry carries e negated (WinTouched); the hot list holds the user rows first, both parts in target order
        size_t qi = (size_t)H.nhot_user, qu = 0;
        for (size_t t = 0; t < (size_t)NT; t++) {
            if (tptr[t + 1] <= tptr[t]) continue;
            bool is_hot;
            if (t < (size_t)(NF + NI)) { is_hot = qi < H.hot.size() && (size_t)NF + (size_t)H.hot[qi].j == t; qi += is_hot; }
            else { is_hot = qu < (size_t)H.nhot_user && (size_t)(NF + NI) + (size_t)H.hot[qu].j == t; qu += is_hot; }
            H.touched.push_back(WinTouched{(int)t, tptr[t], is_hot ? -tptr[t + 1] : tptr[t + 1]});
        }
    }
    for (size_t j = 0; j < nunit; j++) units[j].first = wsegs[(size_t)units[j].seg_begin];   // the first segment travels with the unit record
    H.nrow = nrow; H.nent = nent; H.nfbe = nfbe; H.fixed_ng = fixed_ng; H.unit_uval = unit_uval;
    H.nshared = NS; H.shared_entries = (long)H.uent.size(); H.item_children = (long)H.ient.size();
    if (has_shared && feedback) {   // attributes of the USER: the same section on every row of a segment -- the wave walk keeps it in registers (svdf_k_wave.hip)
        bool same = true;
        for (size_t q = 0; q < nseg_used && same; q++) {
            const int r0 = wsegs[q].row_begin, a0 = H.uptr[(size_t)r0], n0 = H.uptr[(size_t)r0 + 1] - a0;
            same = n0 <= 4;
            for (int r = r0 + 1; r < r0 + wsegs[q].row_count && same; r++) {
                const int a = H.uptr[(size_t)r];
                same = H.uptr[(size_t)r + 1] - a == n0 && H.upos[(size_t)r] == H.upos[(size_t)r0];
                for (int j = 0; j < n0 && same; j++) same = H.uent[(size_t)(a + j)].idx == H.uent[(size_t)(a0 + j)].idx && H.uent[(size_t)(a + j)].val == H.uent[(size_t)(a0 + j)].val;
            }
        }
        H.shared_uniform = same;
    }
    for (long nr = 0; nr < nrow; nr++) { const int g = rptr[(size_t)2 * nr + 1] - rptr[(size_t)2 * nr]; H.global_entries += g; H.item_entries += rptr[(size_t)2 * nr + 2] - rptr[(size_t)2 * nr] - g; }
}
// the uploads and the data set's fields: the calling thread, in window order
void Engine::wunit_adopt(Dataset *ds, const WUnitHost &H) {
    const std::vector<WinUnit> &units = H.units;
    const std::vector<WinSeg> &wsegs = H.wsegs;
    const std::vector<float> &w_label = H.w_label, &w_uval = H.w_uval;
    const std::vector<int> &rptr = H.rptr, &tptr = H.tptr, &gptr = H.gptr;
    const std::vector<WinEnt> &ent = H.ent, &fbent = H.fbent;
    const long nrow = H.nrow, nent = H.nent, nfbe = H.nfbe;
    const size_t nunit = units.size(), nseg_used = wsegs.size();
    const int fixed_ng = H.fixed_ng;
    const bool unit_uval = H.unit_uval;
    if (window_trained_ == ds) window_trained_ = nullptr;
    ds->kind = 7;
    ds->sched_signature = schedule_signature();
    ds->wu_feedback = H.feedback;
    // rptr as the kernel reads it: rptr[2r], rptr[2r + 1], rptr[2r + 2] -- the odd entries are the global / item boundary of row r
    ds->num_row = nrow;
    ds->num_units = (long)nunit;
    ds->win_slots = tptr.back();
    ds->wu_gslots = gptr.back();
    ds->wu_estride = fixed_ng >= 0 ? fixed_ng + 1 : 0;
    ds->unit_values = unit_uval;
    ds->wu_units.upload(units.data(), nunit, stream_);
    ds->wu_segs.upload(wsegs.data(), nseg_used, stream_);
    ds->label.upload(w_label.data(), (size_t)nrow, stream_);
    if (!unit_uval) ds->uval.upload(w_uval.data(), (size_t)nrow, stream_);
    if (ds->wu_estride == 0) ds->wu_rptr.upload(rptr.data(), (size_t)2 * nrow + 1, stream_);
    ds->wu_ent.upload(ent.data(), (size_t)nent, stream_);
    ds->wu_fbent.upload(fbent.data(), (size_t)nfbe, stream_);
    ds->win_has_pos = window_keeps_positions();
    if (ds->win_has_pos) ds->win_pos.upload(H.pos.data(), (size_t)nrow, stream_); else ds->win_pos.release();
    ds->wu_fbrec.upload(H.fbrec.data(), H.fbrec.size(), stream_);
    ds->wu_ntouched = H.has_touched ? (long)H.touched.size() : -1;
    if (H.has_touched) ds->wu_touched.upload(H.touched.data(), H.touched.size(), stream_);
    ds->wu_nseg = (long)nseg_used;
    ds->wu_defer_fb = !H.fbrec.empty();
    ds->wu_tptr.upload(tptr.data(), tptr.size(), stream_);
    ds->wu_gptr.upload(gptr.data(), gptr.size(), stream_);
    ds->wu_nshared = H.nshared;
    ds->wu_shared_uniform = H.shared_uniform;
    if (H.nshared > 0) {
        ds->wu_uptr.upload(H.uptr.data(), H.uptr.size(), stream_);
        ds->wu_upos.upload(H.upos.data(), H.upos.size(), stream_);
        ds->wu_uent.upload(H.uent.data(), H.uent.size(), stream_);
    }
    ds->wu_nhot = H.nhot_user;
    ds->wu_nihot = (long)H.hot.size() - H.nhot_user;
    if (!H.hot.empty()) {
        ds->wu_hot.upload(H.hot.data(), H.hot.size(), stream_);
        ds->wu_hrec.upload(H.hrec.data(), H.hrec.size(), stream_);
    }
    ds->wu_nhrec = (long)H.hrec.size();
    ds->wu_ichild = !H.iptr.empty();
    if (ds->wu_ichild) {
        ds->wu_iptr.upload(H.iptr.data(), H.iptr.size(), stream_);
        ds->wu_ient.upload(H.ient.data(), H.ient.size(), stream_);
    }
    HIPCHECK(hipStreamSynchronize(stream_));   // the host columns go out of scope
    ds->sched.level_ptr = {0, nrow};
    ds->sched.max_level_size = nrow;
    // what the reference's step moves -- per row 8k (nu + ni) + 8 (nu_b + ni) + 8 ng + 16 + 8 (ng + nu + ni), per feedback entry 12k + 20
    const long k = mp_.num_factor, nub = mp_.no_user_bias ? 0 : 1;
    const long item_entries = H.item_entries, global_entries = H.global_entries;
    ds->algorithmic_bytes = nrow * (8 * k + 8 * nub + 16 + 8) + item_entries * (8 * k + 8 + 8) + global_entries * 16 + nfbe * (12 * k + 20) +
                            H.shared_entries * (8 * k + 8 * nub + 8) +  // a shared user entry: its row and bias read and written, id + value
                            H.item_children * (8 * k + 8 + 8);          // a feature_item child: like an item entry
}

// A row's private user entry under amd:shared_user_from = B: its user entries [p1, p2) are exactly ONE id < B (returned: its position) and any number
// of shared ids >= B, none of them twice (seen: scratch); shared entries need fp32 slots.
int64_t Engine::private_user_entry(int64_t p1, int64_t p2, const unsigned *feat_index, std::vector<unsigned> &seen) const {
    int64_t pv = -1;
    seen.clear();
    for (int64_t j = p1; j < p2; j++) {
        const unsigned u = feat_index[j];
        if (u >= (unsigned)mp_.num_user) fail("user feature index exceed bound");
        if (u < shared_user_from_) { check(pv < 0, "window data sets: a row needs exactly one private user entry (id < amd:shared_user_from), this one has two"); pv = j; continue; }
        for (unsigned x : seen) if (x == u) fail("window data sets: a shared user id listed twice in one row");
        seen.push_back(u);
        check(!contrib_bf16_, "window data sets: shared user entries (amd:shared_user_from) need amd:contrib = fp32");
    }
    check(pv >= 0, "window data sets: a row needs exactly one private user entry (id < amd:shared_user_from), this one has none");
    return pv;
}
// ---- one exchange window of rows of a random-order trainer: any number of global and item entries, exactly one user entry
// shared: the one-GPU window sequence under amd:shared_user_from = B -- a row's user entries are ONE private id < B (the unit's user) and any
// number of shared ids >= B (targets like item rows).  Otherwise every row has exactly one user entry.  The sequence also takes loaded
// feature_user / feature_item tables: every child is a shared target, and no row may reach one target twice.
void Engine::wunit_host_from_csr(WUnitHost &H, bool inplace, long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                 const float *feat_value, bool shared, int shared_sub, int item_sub) const {
    const long NU = mp_.num_user;
    const unsigned B = shared_user_from_;
    const bool children = shared && side_tables();
    std::vector<int> cnt((size_t)NU, 0);
    std::vector<int64_t> priv;   // shared mode: the private entry of every row
    if (shared && shared_user()) priv.resize((size_t)n);
    std::vector<unsigned> seen;
    for (long r = 0; r < n; r++) {
        if (children) side_children_ok(row_ptr + 3 * r, feat_index, seen);
        const int64_t p1 = row_ptr[3 * r + 1], p2 = row_ptr[3 * r + 2];
        if (priv.empty()) {
            if (p2 - p1 != 1 && shared_user())
                for (int64_t j = p1; j < p2; j++)
                    check(feat_index[j] < B, "svdf_dataset_window_from_csr: shared user entries (amd:shared_user_from) are for the one-GPU window sequence; "
                                             "the N-rank exchange has no place for user rows");
            check(p2 - p1 == 1, "window data sets: every row needs exactly one user entry");
        } else {
            priv[(size_t)r] = private_user_entry(p1, p2, feat_index, seen);
        }
        const unsigned u = feat_index[priv.empty() ? p1 : priv[(size_t)r]];
        if (u >= (unsigned)NU) fail("user feature index exceed bound");
        cnt[u]++;
    }
    // one segment per active user, in order of first occurrence; its rows in file order
    std::vector<int> seg_of_user((size_t)NU, -1);
    std::vector<HostSeg> segs;
    for (long r = 0; r < n; r++) {
        const unsigned u = feat_index[priv.empty() ? row_ptr[3 * r + 1] : priv[(size_t)r]];
        if (seg_of_user[u] < 0) { seg_of_user[u] = (int)segs.size(); HostSeg h; h.user = u; h.has_user = true; h.row_count = (size_t)cnt[u]; segs.push_back(h); }
    }
    { size_t acc = 0; for (auto &h : segs) { h.row_first = acc; acc += h.row_count; h.row_count = 0; } }
    std::vector<int64_t> seg_rows((size_t)n);
    for (long r = 0; r < n; r++) {
        HostSeg &h = segs[(size_t)seg_of_user[feat_index[priv.empty() ? row_ptr[3 * r + 1] : priv[(size_t)r]]]];
        seg_rows[h.row_first + h.row_count++] = r;
    }
    wunit_build_host(H, inplace, segs.data(), segs.size(), seg_rows, true, n, row_label, row_ptr, feat_index, feat_value, nullptr, nullptr,
                     priv.empty() ? nullptr : priv.data(), children, shared_sub, item_sub);
}
// One row's side-table children (the one-GPU window sequence): a feature_user child is a shared user row (id >= amd:shared_user_from), and
// a child must not reach a row the row already touches (its own entries or an earlier child) -- one contribution per target and row.  Two
// plain entries with one id keep the builder's own messages.
void Engine::side_children_ok(const int64_t *p, const unsigned *feat_index, std::vector<unsigned> &seen) const {
    if (const char *rule = side_children_rule(p, feat_index, seen)) fail(rule);
}
// the same test as a predicate (the staged route decides without raising, svdf_staged.cpp): nullptr, or the message of the rule the row breaks
const char *Engine::side_children_rule(const int64_t *p, const unsigned *feat_index, std::vector<unsigned> &seen) const {
    const unsigned B = shared_user_from_;
    for (int side = 0; side < 2; side++) {
        const SideTable &T = side == 0 ? feat_user_ : feat_item_;
        const int64_t a = p[1 + side], b = p[2 + side];
        if (T.num_row() == 0) continue;
        seen.assign(feat_index + a, feat_index + b);
        for (int64_t j = a; j < b; j++) {
            const unsigned id = feat_index[j];
            if (id >= T.num_row()) continue;
            for (unsigned c = T.row_ptr[id]; c < T.row_ptr[id + 1]; c++) {
                const unsigned x = T.index[c];
                if (side == 0 && x < B)
                    return "window data sets: a feature_user child below amd:shared_user_from (it would be another unit's private user row)";
                for (unsigned y : seen)
                    if (y == x) return side == 0 ? "window data sets: a row reaches one user row twice through feature_user children (each row may touch a target once)"
                                                 : "window data sets: a row reaches one item row twice through feature_item children (each row may touch a target once)";
                seen.push_back(x);
            }
        }
    }
    return nullptr;
}

// ---- one exchange window of a user-group pass: blocks [b0, b1), every START closed by its END inside the window
// shared: the one-GPU window sequence under amd:shared_user_from = B -- a row's user entries are ONE private id < B, the
// same on every row of a block (or START..END span): the unit's user; and any number of shared ids >= B, which may differ from row to row.
void Engine::wunit_host_from_blocks(WUnitHost &H, bool inplace, long b0, long b1, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index,
                                    const float *fb_value, const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr,
                                    const unsigned *feat_index, const float *feat_value, bool shared, int shared_sub, int item_sub) const {
    const long NU = mp_.num_user;
    const long r_lo = block_row_ptr[b0], r_hi = block_row_ptr[b1];
    std::vector<int64_t> priv;   // shared mode: the private entry of every row of the window
    if (shared) priv.resize((size_t)(r_hi - r_lo));
    std::vector<unsigned> seen;
    std::vector<HostSeg> segs;
    std::vector<int64_t> seg_rows;
    bool open = false;
    for (long b = b0; b < b1; b++) {
        const int tag = extend_tag[b];
        check(tag == TAG_DEFAULT || tag == TAG_START || tag == TAG_MIDDLE || tag == TAG_END, "dataset_from_blocks: unknown extend_tag");
        if (tag == TAG_DEFAULT || tag == TAG_START) {
            check(!open, "window data sets: a START block inside an open START..END span");
            HostSeg h;
            h.fb_begin = fb_ptr[b]; h.fb_count = fb_ptr[b + 1] - fb_ptr[b]; h.row_first = seg_rows.size();
            segs.push_back(h);
            open = true;
        } else {
            check(open, "start tag,end tag error in implicit feedback");
        }
        HostSeg &h = segs.back();
        for (int64_t r = block_row_ptr[b]; r < block_row_ptr[b + 1]; r++) {
            const int64_t p1 = row_ptr[3 * r + 1], p2 = row_ptr[3 * r + 2];
            int64_t pv = p1;
            if (priv.empty()) check(p2 - p1 == 1, "window data sets: every row needs exactly one user entry");
            else pv = priv[(size_t)(r - r_lo)] = private_user_entry(p1, p2, feat_index, seen);
            const unsigned u = feat_index[pv];
            if (u >= (unsigned)NU) fail("user feature index exceed bound");
            if (!h.has_user) { h.user = u; h.has_user = true; }
            check(h.user == u, priv.empty() ? "window data sets: the rows of one block (or START..END span) must belong to one user"
                                            : "window data sets: the rows of one block (or START..END span) must belong to one user (one private id < amd:shared_user_from)");
            seg_rows.push_back(r);
            h.row_count++;
        }
        if (tag == TAG_END) {
            const int64_t nf = fb_ptr[b + 1] - fb_ptr[b];
            bool same = nf == h.fb_count;
            for (int64_t j = 0; same && j < nf; j++) same = fb_index[fb_ptr[b] + j] == fb_index[h.fb_begin + j] && fb_value[fb_ptr[b] + j] == fb_value[h.fb_begin + j];
            check(same, "svdfeature_amd: START and END blocks of one user must carry the same feedback list");
        }
        if (tag == TAG_DEFAULT || tag == TAG_END) open = false;
    }
    check(!open, "window data sets: a window must not end inside a START..END span");
    // source row ids relative to the window's first row
    for (auto &r : seg_rows) r -= r_lo;
    std::vector<int64_t> ptr((size_t)3 * (r_hi - r_lo) + 1);
    for (size_t j = 0; j < ptr.size(); j++) ptr[j] = row_ptr[3 * r_lo + (long)j];
    wunit_build_host(H, inplace, segs.data(), segs.size(), seg_rows, false, r_hi - r_lo, row_label + r_lo, ptr.data(), feat_index, feat_value, fb_index, fb_value,
                     priv.empty() ? nullptr : priv.data(), false, shared_sub, item_sub);
}

Dataset *Engine::dataset_window_from_csr(long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value) {
    wunit_check_config("dataset_window_from_csr");
    need_device("dataset");
    check(!user_group(), "svdf_dataset_window_from_csr: random-order (format_type 0) trainers; user-group data goes through svdf_dataset_window_from_blocks");
    check(!multi_ || in_multi_scope(), "window data sets are per rank; an amd:gpus handle builds them itself from svdf_dataset_from_csr");
    validate_csr_pointers(n, row_ptr);
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get());
    WUnitHost H;
    wunit_host_from_csr(H, false, n, row_label, row_ptr, feat_index, feat_value);
    wunit_adopt(ds.get(), H);
    return ds.release();
}
Dataset *Engine::dataset_window_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                            const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                            const float *feat_value) {
    wunit_check_config("dataset_window_from_blocks");
    need_device("dataset");
    check(user_group(), "svdf_dataset_window_from_blocks: user-group (format_type 1) trainers");
    check(!multi_ || in_multi_scope(), "window data sets are per rank; an amd:gpus handle builds them itself from svdf_dataset_from_blocks");
    validate_block_pointers(num_block, fb_ptr, block_row_ptr);
    validate_csr_pointers((long)(block_row_ptr[num_block] - block_row_ptr[0]), row_ptr + 3 * block_row_ptr[0]);
    if (shared_user())   // a row with several user entries, one of them shared: the cause is named before the builder's "exactly one user entry"
        for (int64_t r = block_row_ptr[0]; r < block_row_ptr[num_block]; r++)
            if (row_ptr[3 * r + 2] - row_ptr[3 * r + 1] != 1)
                for (int64_t j = row_ptr[3 * r + 1]; j < row_ptr[3 * r + 2]; j++)
                    check(feat_index[j] < shared_user_from_, "svdf_dataset_window_from_blocks: shared user entries (amd:shared_user_from) are for the one-GPU window "
                                                             "sequence; the N-rank exchange has no place for user rows");
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get());
    WUnitHost H;
    wunit_host_from_blocks(H, false, 0, num_block, extend_tag, fb_ptr, fb_index, fb_value, block_row_ptr, row_label, row_ptr, feat_index, feat_value);
    wunit_adopt(ds.get(), H);
    return ds.release();
}

// first half of the step on a kind-7 data set (train_dataset): the users' walks; the contributions stay in the trainer's scratch
void Engine::wunit_train(Dataset *ds) {
    d_contrib_.reserve((size_t)std::max<long>(ds->win_slots, 1) * (size_t)pitch_);
    d_cbias_.reserve((size_t)std::max<long>(ds->win_slots, 1));
    d_gcontrib_.reserve((size_t)std::max<long>(ds->wu_gslots, 1));
    if (ds->wu_feedback && ds->wu_nhot + ds->wu_nihot > 0) { d_hfb_.reserve((size_t)std::max<long>(ds->wu_nhrec, 1) * (size_t)pitch_); d_hfbb_.reserve((size_t)std::max<long>(ds->wu_nhrec, 1)); }
    if (ds->wu_defer_fb) { d_dvec_.reserve((size_t)std::max<long>(ds->wu_nseg, 1) * (size_t)pitch_); d_dbias_.reserve((size_t)std::max<long>(ds->wu_nseg, 1)); }
    const int form = launch_wunit_walk(params(), wunit_view(ds), ds->wu_feedback, wunit_fast_, stream_, ds->wu_shared_uniform);
    if (form == 1) n_wave_shared_++;                                            // counter 33
    else if (ds->wu_feedback && ds->wu_nshared > 0) n_walk_shared_++;           // counter 34
    window_trained_ = ds;
}
// second half: dst == nullptr adds the per-target sums to the model in place, else they go to the wire buffer
void Engine::wunit_sum(Dataset *ds, void *dst, int half) {
    launch_wunit_sum(params(), wunit_view(ds), dst, half, stream_);
}

void validate_csr_pointers(long num_row, const int64_t *row_ptr) {
    check(num_row >= 0, "dataset: negative row count");
    if (num_row == 0) return;
    check(row_ptr[0] >= 0, "CSR row_ptr must not be negative");
    for (long r = 0; r < num_row; r++) {
        const int64_t *p = &row_ptr[(size_t)3 * r];
        check(p[0] <= p[1] && p[1] <= p[2] && p[2] <= p[3], "CSR row_ptr must be non-decreasing");
    }
    check(row_ptr[(size_t)3 * num_row] - row_ptr[0] < (int64_t)2147483647, "dataset: more than 2^31-1 feature entries");
}
void validate_block_pointers(long num_block, const int64_t *fb_ptr, const int64_t *block_row_ptr) {
    check(num_block >= 0, "dataset_from_blocks: negative block count");
    check(fb_ptr[0] >= 0 && block_row_ptr[0] >= 0, "dataset_from_blocks: block_row_ptr / fb_ptr must not be negative");
    for (long b = 0; b < num_block; b++)
        check(block_row_ptr[b] <= block_row_ptr[b + 1] && fb_ptr[b] <= fb_ptr[b + 1], "dataset_from_blocks: block_row_ptr / fb_ptr must be non-decreasing");
    check(fb_ptr[num_block] - fb_ptr[0] < (int64_t)2147483647 && block_row_ptr[num_block] - block_row_ptr[0] < (int64_t)2147483647,
          "dataset_from_blocks: more than 2^31-1 rows / feedback entries");
}
static bool no_id_twice(const unsigned *a, int64_t n, std::vector<unsigned> &tmp) {
    if (n < 2) return true;
    if (n <= 8) { for (int64_t i = 0; i < n; i++) for (int64_t j = i + 1; j < n; j++) if (a[i] == a[j]) return false; return true; }
    tmp.assign(a, a + n);
    std::sort(tmp.begin(), tmp.end());
    return std::adjacent_find(tmp.begin(), tmp.end()) == tmp.end();
}
// shared_from (amd:shared_user_from, one-GPU window sequences): a row's user entries are one id < shared_from and shared ids, none twice
bool wunit_rows_ok(long r0, long r1, const int64_t *row_ptr, const unsigned *feat_index, unsigned shared_from) {
    std::vector<unsigned> tmp;
    for (long r = r0; r < r1; r++) {
        const int64_t *p = &row_ptr[(size_t)3 * r];
        if (shared_from != 0xFFFFFFFFu && p[2] > p[1] + 1) {
            int priv = 0;
            for (int64_t j = p[1]; j < p[2]; j++) priv += feat_index[j] < shared_from;
            if (priv != 1 || !no_id_twice(feat_index + p[1], p[2] - p[1], tmp)) return false;
        } else if (p[2] != p[1] + 1) return false;
        if (shared_from != 0xFFFFFFFFu && feat_index[p[1]] >= shared_from && p[2] == p[1] + 1) return false;
        if (!no_id_twice(feat_index + p[0], p[1] - p[0], tmp) || !no_id_twice(feat_index + p[2], p[3] - p[2], tmp)) return false;
    }
    return true;
}
bool wunit_blocks_one_user_entry(long num_block, const int64_t *block_row_ptr, const int64_t *row_ptr) {
    for (int64_t r = block_row_ptr[0]; r < block_row_ptr[num_block]; r++)
        if (row_ptr[(size_t)3 * r + 2] - row_ptr[(size_t)3 * r + 1] != 1) return false;
    return true;
}
bool wunit_blocks_ok(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const int64_t *block_row_ptr,
                     const int64_t *row_ptr, const unsigned *feat_index, unsigned shared_from) {
    std::vector<unsigned> tmp;
    bool open = false, have_user = false;
    unsigned user = 0;
    for (long b = 0; b < num_block; b++) {
        const int tag = extend_tag[b];
        if (tag == TAG_DEFAULT || tag == TAG_START) { if (open) return false; have_user = false; }
        else if (tag == TAG_MIDDLE || tag == TAG_END) { if (!open) return false; }
        else return false;
        if (!no_id_twice(fb_index + fb_ptr[b], fb_ptr[b + 1] - fb_ptr[b], tmp)) return false;
        if (!wunit_rows_ok((long)block_row_ptr[b], (long)block_row_ptr[b + 1], row_ptr, feat_index, shared_from)) return false;
        for (int64_t r = block_row_ptr[b]; r < block_row_ptr[b + 1]; r++) {
            int64_t pv = row_ptr[(size_t)3 * r + 1];   // the private entry (wunit_rows_ok: exactly one below shared_from)
            if (shared_from != 0xFFFFFFFFu) while (feat_index[(size_t)pv] >= shared_from) pv++;
            const unsigned u = feat_index[(size_t)pv];
            if (have_user && u != user) return false;
            user = u; have_user = true;
        }
        open = (tag == TAG_START || tag == TAG_MIDDLE);
    }
    return !open;
}

}  // namespace svdf

// svdf_staged.cpp -- `amd:step = minibatch | auto` on the staged route (svdf_update_csr / _csr_batch / _block) of a one-GPU handle.
// DESIGN.md section 6l.  A chunk -- the rows staged between two flush points -- is trained as the window sequence that
// svdf_dataset_from_{triples,pairs,csr,blocks} would build from the same rows on the same handle state: the builders, the window rule and
// the kernels are the resident ones (svdf_wunit.cpp, svdf_window.cpp), nothing here computes on parameters.  What is new per chunk is the
// recurring build: the transient sequence's device blocks come from and go back to a pool kept on the handle (DevPool) instead of
// hipMalloc / hipFree.  Chunks the window step does not cover are decided WITHOUT raising (a CLI run that trains today must not stop mid-round
// because a key was added) and keep the exact flush; the first one says so on stderr.
#include "svdf_engine.h"

#include <cmath>
#include <cstring>
#include <memory>

#include "svdf_internal.h"
#include "svdf_kernels.h"

namespace svdf {

// ---- the handle's cache of device blocks
static thread_local DevPool *tl_dev_pool = nullptr;
DevPool *dev_pool_current() { return tl_dev_pool; }
DevPoolScope::DevPoolScope(DevPool *p) : prev(tl_dev_pool) { tl_dev_pool = p; }
DevPoolScope::~DevPoolScope() { tl_dev_pool = prev; }
void DevPool::drop() {
    for (auto &kv : blocks) (void)hipFree(kv.second.p);
    blocks.clear();
}
// the smallest cached block that holds `bytes` and is at most twice as large (a chunk's buffers repeat their sizes; a remainder chunk must
// not pin the large blocks under small requests)
void *DevPool::take(size_t bytes, size_t &got) {
    auto it = blocks.lower_bound(bytes);
    if (it == blocks.end() || it->first > 2 * bytes + 4096) { n_missed++; return nullptr; }
    void *p = it->second.p;
    got = it->first;
    blocks.erase(it);
    n_taken++;
    return p;
}
void DevPool::give(void *p, size_t bytes) { blocks.emplace(bytes, Block{p, gen}); }
// a block handed back during chunk g carries gen g; one that nobody took since chunk g - 2 goes back to the device
void DevPool::end_chunk() {
    gen++;
    for (auto it = blocks.begin(); it != blocks.end();) {
        if (it->second.gen + 2 < gen) { (void)hipFree(it->second.p); it = blocks.erase(it); }
        else ++it;
    }
}

// ---- what keeps a configuration out of the window step: wunit_check_config / window_build_header as a predicate
// user_units: the chunk takes the user-unit kernels (rows with globals or several entries, SVD++ blocks: num_factor <= 256); chunks of plain ratings / rank
// pairs take the window kernels, which have wide rows
const char *Engine::staged_config_rule(bool blocks, bool user_units) const {
    if (mtype_.extend_type != 0) return "the window step covers the base solvers only (extend_type 0)";
    if (relaxed()) return "relaxed ids (amd:relax_*) are outside the window step";
    if (lazy_decay()) return "lazy decay (reg_method / reg_global >= 4) is outside the window step";
    if (mp_.common_latent_space != 0) return "a shared latent space (common_latent_space) is outside the window step";
    if (g_stride_ != 1) return "the relaxed layout of the global biases is outside the window step";
    if (user_units && !wunit_width_ok()) return "the window step of rows with global features, several user / item entries or implicit feedback needs num_factor <= 256";
    if (side_tables()) {
        if (blocks) return "feature_user / feature_item side tables are not supported with user-group (SVD++) trainers in the window step";
        if (feat_user_.num_row() != 0 && !shared_user()) return "a feature_user side table needs amd:shared_user_from in the window step (its children are shared user rows)";
        if (contrib_bf16_) return "feature_user / feature_item side tables need amd:contrib = fp32 in the window step";
    }
    if (wseq_shared_sub_ > 0) {
        if (contrib_bf16_) return "window_shared_sub > 0 needs amd:contrib = fp32";
        if (blocks) return "window_shared_sub > 0 is not supported with user-group (SVD++) trainers";
        if (shared_user() && wunit_inplace_ == 0) return "window_shared_sub > 0 (ordered sub-steps for shared user rows) needs the in-place sums (knob wunit_inplace = 1)";
    }
    if (wseq_item_sub_ > 0) {
        if (contrib_bf16_) return "window_item_sub > 0 needs amd:contrib = fp32";
        if (blocks) return "window_item_sub > 0 is not supported with user-group (SVD++) trainers";
        if (wunit_inplace_ == 0) return "window_item_sub > 0 (ordered sub-steps for hot item rows) needs the in-place sums (knob wunit_inplace = 1)";
    }
    if (blocks && block_sub() > 0 && contrib_bf16_) return "window_block_sub > 0 needs amd:contrib = fp32";
    if (blocks && block_item_sub() > 0) {
        if (contrib_bf16_) return "window_block_item_sub > 0 needs amd:contrib = fp32";
        if (wunit_inplace_ == 0) return "window_block_item_sub > 0 (ordered sub-steps for hot item rows of SVD++ blocks) needs the in-place sums (knob wunit_inplace = 1)";
    }
    if (wseq_pair_sub_ > 0) {
        if (contrib_bf16_) return "window_pair_sub > 0 needs amd:contrib = fp32";
        if (blocks) return "window_pair_sub > 0 is not supported with user-group (SVD++) trainers";
        if (!wunit_width_ok()) return "window_pair_sub > 0 needs num_factor <= 256";
    }
    if (blocks && mp_.common_feedback_space != 0) return "user-group trainers need a feedback space of their own (common_feedback_space = 0) in the window step";
    if (shared_user() && !(shared_user_from_ >= 1 && (long)shared_user_from_ <= (long)mp_.num_user)) return "amd:shared_user_from must be in 1 .. num_user";
    return nullptr;
}

void Engine::staged_keep_exact(const char *rule) {
    n_staged_exact_++;
    staged_pool_.end_chunk();   // a handle whose chunks stay exact gives the cached blocks back
    if (staged_exact_said_) return;
    staged_exact_said_ = true;
    if (getenv("SVDF_QUIET")) return;
    fprintf(stderr, "[svdfeature_amd] amd:step = %s: a chunk of staged rows keeps the exact (level-scheduled) step: %s.  Later chunks like it stay exact without another line "
                    "(counter 31 counts them).\n", step_auto_set_ ? "auto" : "minibatch", rule);
}

// The guard of the DEFAULT step (note_dataset's, for chunks of the staged route): the exact schedule this flush has just built against the
// streaming model; the line names `amd:step = auto` once per handle.
void Engine::staged_guard(long n, long levels, double unit_us, long bytes) {
    if (n_staged_guard_ > 0 || step_auto_set_ || step_minibatch_set_ || multi_ || gpus_ != 1 || is_peer_ || host_only_) return;
    const double dag_ms = (double)levels * unit_us * 1e-3;
    if (dag_ms < 50.0) return;   // (chunks below 50 ms are not worth a line: note_dataset's floor)
    const double stream_ms = (double)bytes / (0.57 * 8.0e12) * 1e3;
    if (dag_ms <= 10.0 * stream_ms) return;
    n_staged_guard_++;
    if (getenv("SVDF_QUIET")) return;
    fprintf(stderr, "[svdfeature_amd] default (exact) step on staged rows (svdf_update_*): a chunk of %ld rows in %ld conflict-free levels -- the data's dependency depth "
                    "binds: about %.0f ms per chunk (%.2f M rows/s; levels x %.1f us) against %.1f ms if the rows streamed.  The exact step keeps the reference's "
                    "sequential result bit for bit; `amd:step = auto` would train such chunks with the window step (user side exact, shared rows once per window; "
                    "|dRMSE| <= 1e-4 contract) where it covers the configuration\n",
            n, levels, dag_ms, (double)n / dag_ms * 1e-3, unit_us, stream_ms);
}

// trains and drops a transient window sequence: what svdf_train_dataset does for a kind-8 data set, without its flush (this IS the flush)
void Engine::staged_train(Dataset *seq) {
    std::unique_ptr<Dataset> ds(seq);
    wseq_train(ds.get());
    HIPCHECK(hipGetLastError());
    n_batches_ += (int64_t)ds->wchild.size();
    n_instances_ += ds->num_row;
    sample_counter_ += (unsigned)ds->num_row;
    n_flushes_++;
    n_staged_window_++;
}

// `amd:step = auto`, first chunk of at least device_schedule_min rows: the existing estimator (auto_step) on the chunk's exact level count.
// true: the window step was chosen and `out` is the built sequence.  The decision stays until set_param.
bool Engine::staged_auto_decide(long n, int kind, long units, long levels, long bytes, const char *rule, const std::function<Dataset *()> &build_window, Dataset *&out) {
    const bool window_ok = rule == nullptr;
    Dataset *probe = new Dataset();   // what auto_step measures: schedule depth, unit count, algorithmic bytes (never adopted, no device memory)
    probe->kind = kind; probe->num_row = n; probe->num_units = units; probe->algorithmic_bytes = bytes;
    probe->sched.level_ptr.assign((size_t)levels + 1, 0);
    Dataset *got = auto_step(probe, window_ok, build_window);
    staged_auto_decision_ = auto_last_.decided;
    if (auto_last_.decided == 2) { out = got; return true; }
    if (auto_last_.decided == 3) { staged_auto_rule_ = rule ? rule : ""; staged_keep_exact(staged_auto_rule_.c_str()); }   // deep, but outside the window step: counted and said like under minibatch
    delete got;
    return false;
}

static inline long row_bytes(int k, int nb, long rows_ui, long nnz) { return 8L * k * rows_ui + 8L * nb + 16 + 8 * nnz; }

// ---- random-order trainers: flush_csr's chunk
bool Engine::staged_window_csr(HostCSR &src) {
    const long n = src.num_row();
    const bool auto_mode = step_auto_set_;
    if (auto_mode && staged_auto_decision_ == 3) { staged_keep_exact(staged_auto_rule_.c_str()); return false; }
    if (auto_mode && staged_auto_decision_ != 0 && staged_auto_decision_ != 2) return false;   // exact kept: the default flush, bit for bit
    if (auto_mode && staged_auto_decision_ == 0 && n < device_sched_min_) return false;       // too small to judge: exact, undecided
    need_device("update");
    std::unique_ptr<ScopedNs> build_timer(new ScopedNs(ns_staged_build_));   // pre-check + build + upload, until the sequence is ready to train
    const int *rp = src.row_ptr.data();
    const unsigned *idx = src.feat_index.data();
    const float *val = src.feat_value.data();
    // the chunk's shape picks the builder svdf_dataset_from_* would be called with
    bool triples = window_rows_allowed(), pairs = triples;
    for (long r = 0; r < n && (triples || pairs); r++) {
        const int *p = rp + 3 * r;
        if (p[1] != p[0] || p[2] != p[1] + 1) { triples = pairs = false; break; }
        if (triples) triples = p[3] == p[2] + 1 && val[p[1]] == 1.0f && val[p[2]] == 1.0f;
        if (pairs) {   // the generator's shape (punit_flush's test): user:1, {lower item id: +-1, higher: -+1}, label 1
            pairs = p[3] == p[2] + 2 && src.row_label[(size_t)r] == 1.0f && val[p[1]] == 1.0f && (val[p[2]] == 1.0f || val[p[2]] == -1.0f) &&
                    val[p[2] + 1] == -val[p[2]] && idx[p[2]] < idx[p[2] + 1];
        }
    }
    if (n == 0) triples = pairs = false;
    const char *rule = staged_config_rule(false, !triples && !pairs);
    std::vector<int64_t> ptr64;
    if (!triples && !pairs) {
        ptr64.assign(src.row_ptr.begin(), src.row_ptr.end());
        if (!rule) {   // the rows the builders refuse (wunit_host_from_csr): decided here, without raising
            const unsigned B = shared_user_from_;
            std::vector<unsigned> seen;
            const bool children = side_tables();
            for (long r = 0; r < n && !rule; r++) {
                const int64_t *p = &ptr64[(size_t)3 * r];
                if (shared_user()) {
                    int priv = 0;
                    for (int64_t j = p[1]; j < p[2]; j++) priv += idx[j] < B;
                    if (priv != 1) rule = "a row needs exactly one private user entry (id < amd:shared_user_from)";
                    else if (p[2] - p[1] > 1 && contrib_bf16_) rule = "shared user entries (amd:shared_user_from) need amd:contrib = fp32";
                } else if (p[2] - p[1] != 1) rule = "every row needs exactly one user entry (amd:shared_user_from declares shared user ids)";
                if (!rule && !wunit_rows_ok(r, r + 1, ptr64.data(), idx, shared_user() ? B : 0xFFFFFFFFu)) rule = "a row lists one global, user or item id twice";
                if (!rule && children) rule = side_children_rule(p, idx, seen);
            }
        }
    }
    // the builders read the chunk through columns / 64-bit pointers; they copy everything they keep
    std::vector<unsigned> cu, c0, c1;
    auto build = [&]() -> Dataset * {
        staged_building_ = true;   // a transient sequence, dropped after its one pass: its windows keep no file positions
        struct Done { bool &f; ~Done() { f = false; } } done{staged_building_};
        if (triples || pairs) {
            cu.resize((size_t)n); c0.resize((size_t)n);
            if (pairs) c1.resize((size_t)n);
            for (long r = 0; r < n; r++) {
                const int *p = rp + 3 * r;
                cu[(size_t)r] = idx[p[1]];
                if (triples) c0[(size_t)r] = idx[p[2]];
                else {   // pos = the +1 item
                    const bool lo_pos = val[p[2]] == 1.0f;
                    c0[(size_t)r] = idx[p[2] + (lo_pos ? 0 : 1)]; c1[(size_t)r] = idx[p[2] + (lo_pos ? 1 : 0)];
                }
            }
            return triples ? wseq_from_triples(n, cu.data(), c0.data(), src.row_label.data()) : wseq_from_pairs(n, cu.data(), c0.data(), c1.data());
        }
        return wseq_from_csr(n, src.row_label.data(), ptr64.data(), idx, val);
    };
    DevPoolScope pool(staged_pool_mode_ ? &staged_pool_ : nullptr);
    Dataset *seq = nullptr;
    if (auto_mode && staged_auto_decision_ == 0) {
        // the chunk's exact level count on a scratch tracker (the schedule flush_csr builds anyway, relative to an empty history)
        LevelTracker scratch;
        scratch.resize(num_resources() + 1);
        std::swap(scratch, tracker_);
        long levels = 0, bytes = 0;
        const int nb = mp_.no_user_bias ? 1 : 2;
        for (long r = 0; r < n; r++) {
            const int *p = rp + 3 * r;
            const int lvl = level_of_row(idx + p[0], p[1] - p[0], idx + p[1], p[2] - p[1], idx + p[2], p[3] - p[2], 0) + 1;
            touch_row(idx + p[0], p[1] - p[0], idx + p[1], p[2] - p[1], idx + p[2], p[3] - p[2], lvl);
            levels = std::max<long>(levels, lvl);
            bytes += row_bytes(mp_.num_factor, nb, p[3] - p[1], p[3] - p[0]);
        }
        std::swap(scratch, tracker_);
        int kind = 2;
        long units = n;
        if (pairs && n >= 64 && punit_config_ok() && pair_units_applies(params())) {
            // a user-grouped pair chunk: the exact flush would walk it as user-run units (punit_flush) -- judged on THAT schedule
            std::vector<unsigned> pu((size_t)n), lo((size_t)n), hi((size_t)n);
            for (long r = 0; r < n; r++) { const int *p = rp + 3 * r; pu[(size_t)r] = idx[p[1]]; lo[(size_t)r] = idx[p[2]]; hi[(size_t)r] = idx[p[2] + 1]; }
            std::vector<PairUnit> sorted;
            std::vector<long> lptr;
            if (punit_build(n, pu.data(), lo.data(), hi.data(), sorted, lptr)) {
                kind = 11; units = (long)sorted.size(); levels = (long)lptr.size() - 1;
                bytes = n * (8L * mp_.num_factor * 3 + 8 * ((mp_.no_user_bias ? 0 : 1) + 2) + 16 + 8 * 3);
            }
        }
        if (!staged_auto_decide(n, kind, units, levels, bytes, rule, build, seq)) return false;
    } else {
        if (rule) { staged_keep_exact(rule); return false; }
        seq = build();
    }
    HIPCHECK(hipStreamSynchronize(stream_));   // the builders' uploads read host arrays that end with this call
    build_timer.reset();
    staged_train(seq);
    staged_pool_.end_chunk();
    src.clear();
    return true;
}

// ---- user-group trainers: flush_units' chunk.  Closed units (START .. END staged here) go through wseq_from_blocks with the blocks as they were
// handed over; a unit that continues one flushed earlier (first) or is still open (last) keeps today's exact unit path, in file order.
bool Engine::staged_window_units() {
    const long nu = (long)staged_units_.size();
    const bool auto_mode = step_auto_set_;
    if (auto_mode && staged_auto_decision_ == 3) { staged_keep_exact(staged_auto_rule_.c_str()); return false; }
    if (auto_mode && staged_auto_decision_ != 0 && staged_auto_decision_ != 2) return false;
    if (auto_mode && staged_auto_decision_ == 0 && staged_.num_row() < device_sched_min_) return false;
    need_device("update");
    std::unique_ptr<ScopedNs> build_timer(new ScopedNs(ns_staged_build_));
    auto closed = [&](long t) { const int f = staged_units_[(size_t)t].flags; return (f & UNIT_START) && (f & UNIT_END); };
    long u0 = 0, u1 = nu;
    if (!closed(0)) u0 = 1;
    if (nu > u0 && !closed(nu - 1)) u1 = nu - 1;
    const char *rule = staged_config_rule(true, true);
    for (long t = 0; t < nu && !rule; t++) {   // rows staged without a block carry neither tag (update_csr_batch marks them UNIT_LOAD | UNIT_SAVE)
        const int f = staged_units_[(size_t)t].flags;
        if (!(f & UNIT_START) && !(f & UNIT_END) && (f & UNIT_SAVE)) rule = "rows without a block (svdf_update_csr on a user-group trainer) are outside the window step";
    }
    // a forced flush that holds only an open user, or only the continuation of one flushed earlier: nothing for a window sequence, the exact
    // unit path as designed -- not a chunk "outside the window step", so neither counted nor announced
    if (!rule && u1 <= u0) return false;
    for (long t = u0; t < u1 && !rule; t++) if (!closed(t)) rule = "a user's START .. END span is interleaved with other units in the chunk";
    if (!rule && u0 == 1 && !(staged_units_[0].flags & UNIT_END)) rule = "a user's START .. END span is interleaved with other units in the chunk";
    // the closed units' blocks in the layout of svdf_dataset_from_blocks
    std::vector<int> tag;
    std::vector<int64_t> fbp{0}, brp, ptr64;
    std::vector<unsigned> fbi;
    std::vector<float> fbv;
    if (!rule) {
        for (const StagedBlk &k : staged_blks_w_) {
            if (k.unit < u0 || k.unit >= u1) continue;
            const HostUnit &u = staged_units_[(size_t)k.unit];
            tag.push_back(k.tag);
            if (brp.empty()) brp.push_back(k.row_begin);
            brp.push_back(k.row_end);
            if (k.tag != TAG_MIDDLE) {   // START / DEFAULT: the prepare list; END: the same list (checked when the block was staged)
                fbi.insert(fbi.end(), staged_fb_index_.begin() + u.fb_begin, staged_fb_index_.begin() + u.fb_end);
                fbv.insert(fbv.end(), staged_fb_value_.begin() + u.fb_begin, staged_fb_value_.begin() + u.fb_end);
            }
            fbp.push_back((int64_t)fbi.size());
        }
        ptr64.assign(staged_.row_ptr.begin(), staged_.row_ptr.end());
        if (tag.empty() || !wunit_blocks_ok((long)tag.size(), tag.data(), fbp.data(), fbi.data(), brp.data(), ptr64.data(), staged_.feat_index.data(), shared_user_for_auto()))
            rule = shared_user() ? "a block's rows or feedback list are outside the window step (one private user id per row and START .. END span, no id twice)"
                                 : "a block's rows or feedback list are outside the window step (one user entry per row, one user per START .. END span, no id twice)";
        else if (shared_user() && !wunit_blocks_one_user_entry((long)tag.size(), brp.data(), ptr64.data()))
            rule = "rows with shared user ids (amd:shared_user_from) on a user-group trainer keep the exact pass on the staged route; the window step trains "
                   "them from resident data sets (svdf_dataset_from_blocks) under amd:step = minibatch";
    }
    auto build = [&]() -> Dataset * {
        staged_building_ = true;   // a transient sequence, dropped after its one pass: its windows keep no file positions
        struct Done { bool &f; ~Done() { f = false; } } done{staged_building_};
        return wseq_from_blocks((long)tag.size(), tag.data(), fbp.data(), fbi.data(), fbv.data(), brp.data(), staged_.row_label.data(), ptr64.data(),
                                staged_.feat_index.data(), staged_.feat_value.data());
    };
    DevPoolScope pool(staged_pool_mode_ ? &staged_pool_ : nullptr);
    Dataset *seq = nullptr;
    if (auto_mode && staged_auto_decision_ == 0) {
        // the exact unit schedule of the whole chunk on a scratch tracker (flush_units builds the same one relative to its history)
        LevelTracker scratch;
        std::swap(scratch, tracker_);
        Schedule sched;
        std::vector<DevUnit> du;
        schedule_units(0, sched, du);
        std::swap(scratch, tracker_);
        const long nb = mp_.no_user_bias ? 1 : 2;
        const long bytes = staged_.num_row() * (8L * mp_.num_factor * 2 + 8 * nb + 16 + 16) + (long)staged_fb_index_.size() * (12L * mp_.num_factor + 20);
        if (!staged_auto_decide(staged_.num_row(), 3, nu, (long)sched.num_levels(), bytes, rule, build, seq)) return false;
    } else {
        if (rule) { staged_keep_exact(rule); return false; }
        seq = build();
    }
    HIPCHECK(hipStreamSynchronize(stream_));
    build_timer.reset();
    // file order: the continued unit (exact), the closed units (window sequence), the open unit (exact)
    struct Piece { HostCSR csr; std::vector<HostUnit> units; std::vector<unsigned> fbi; std::vector<float> fbv; };
    auto cut = [&](long t, Piece &P) {
        HostUnit u = staged_units_[(size_t)t];
        const int e0 = staged_.row_ptr[(size_t)3 * u.row_begin], e1 = staged_.row_ptr[(size_t)3 * u.row_end];
        P.csr.row_label.assign(staged_.row_label.begin() + u.row_begin, staged_.row_label.begin() + u.row_end);
        P.csr.row_ptr.assign(1, 0);
        for (long j = 3L * u.row_begin + 1; j <= 3L * u.row_end; j++) P.csr.row_ptr.push_back(staged_.row_ptr[(size_t)j] - e0);
        P.csr.feat_index.assign(staged_.feat_index.begin() + e0, staged_.feat_index.begin() + e1);
        P.csr.feat_value.assign(staged_.feat_value.begin() + e0, staged_.feat_value.begin() + e1);
        P.fbi.assign(staged_fb_index_.begin() + u.fb_begin, staged_fb_index_.begin() + u.fb_end);
        P.fbv.assign(staged_fb_value_.begin() + u.fb_begin, staged_fb_value_.begin() + u.fb_end);
        u.row_end -= u.row_begin; u.row_begin = 0; u.fb_end -= u.fb_begin; u.fb_begin = 0;
        P.units.assign(1, u);
    };
    Piece head, tail;
    if (u0 == 1) cut(0, head);
    if (u1 < nu) cut(u1, tail);
    auto exact = [&](Piece &P) {
        staged_.row_label.swap(P.csr.row_label); staged_.row_ptr.swap(P.csr.row_ptr); staged_.feat_index.swap(P.csr.feat_index); staged_.feat_value.swap(P.csr.feat_value);
        staged_units_.swap(P.units); staged_fb_index_.swap(P.fbi); staged_fb_value_.swap(P.fbv);
        staged_blks_w_.clear();
        flush_units_exact();
    };
    std::unique_ptr<Dataset> keep(seq);
    if (u0 == 1) exact(head);
    staged_train(keep.release());
    staged_.clear(); staged_units_.clear(); staged_fb_index_.clear(); staged_fb_value_.clear(); staged_blks_w_.clear();
    if (u1 < nu) exact(tail);
    staged_pool_.end_chunk();
    return true;
}

}  // namespace svdf

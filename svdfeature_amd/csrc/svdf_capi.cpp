// svdf_capi.cpp -- extern "C" surface of include/svdfeature_amd.h over svdf::Engine.
#include <svdfeature_amd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "svdf_engine.h"
#include "svdf_kernels.h"
#include "svdf_itemtopn_lists.h"
#include "svdf_ranklines_lists.h"
#include "svdf_pairhard_lists.h"
#include "svdf_ranknegs_lists.h"
#include "svdf_wseq_rule.h"

namespace svdf {
void rank_eval_metrics(long S, const int64_t *sec_ptr, const int *position, const int *ranked, const int *nan, int num_at, const int *at,
                       svdf_rank_metrics *out);
void set_error_mode(int m);
const char *last_error();
void note_error(const std::string &m);
}  // namespace svdf

struct svdf_trainer { svdf::Engine *e; };
struct svdf_dataset { svdf::Dataset *d; };
struct svdf_ranker { svdf::Ranker *r; };
struct svdf_pair_source { svdf::PairSource *s; };

// In error mode 0 svdf::fail() has already printed and exited (reference behaviour); in mode 1 it
// throws and the wrapper turns that into a status code.
#define SVDF_GUARD(retval, ...)                                 \
    try { __VA_ARGS__; }                                        \
    catch (const std::exception &ex) { svdf::note_error(ex.what()); return retval; } \
    catch (...) { svdf::note_error("unknown error"); return retval; }

extern "C" {

const char *svdf_version(void) { return "svdfeature_amd 0.1 (gfx950)"; }
void svdf_set_error_mode(int mode) { svdf::set_error_mode(mode); }
const char *svdf_last_error(void) { return svdf::last_error(); }
int svdf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

svdf_trainer *svdf_create(uint8_t format_type, uint8_t active_type, uint8_t extend_type, uint8_t variant_type, int device) {
    SVDF_GUARD(nullptr, {
        svdf::TypeParam tp{format_type, active_type, extend_type, variant_type};
        svdf_trainer *t = new svdf_trainer();
        t->e = nullptr;
        try { t->e = new svdf::Engine(tp, device); } catch (...) { delete t; throw; }
        return t;
    })
}
void svdf_destroy(svdf_trainer *t) {
    if (!t) return;
    try { delete t->e; } catch (...) {}
    delete t;
}
int svdf_set_param(svdf_trainer *t, const char *name, const char *val) { SVDF_GUARD(-1, { t->e->set_param(name, val); return 0; }) }
void svdf_seed(unsigned seed) { srand(seed); }
int svdf_init_model(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->init_model(); return 0; }) }
int svdf_load_model(svdf_trainer *t, FILE *fi) { SVDF_GUARD(-1, { t->e->load_model(fi); return 0; }) }
int svdf_save_model(svdf_trainer *t, FILE *fo) { SVDF_GUARD(-1, { t->e->save_model(fo); return 0; }) }
int svdf_save_model_begin(svdf_trainer *t, FILE *fo) { SVDF_GUARD(-1, { t->e->save_model_begin(fo); return 0; }) }
int svdf_save_model_end(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->save_model_end(); return 0; }) }
int svdf_init_trainer(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->init_trainer(); return 0; }) }
int svdf_set_round(svdf_trainer *t, int nround) { SVDF_GUARD(-1, { t->e->set_round(nround); return 0; }) }
int svdf_finish_round(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->finish_round(); return 0; }) }

int svdf_update_csr(svdf_trainer *t, float label, int ng, int nu, int ni, const unsigned *index, const float *value) {
    SVDF_GUARD(-1, { t->e->update_csr(label, ng, nu, ni, index, value); return 0; })
}
float svdf_predict_csr(svdf_trainer *t, float label, int ng, int nu, int ni, const unsigned *index, const float *value) {
    SVDF_GUARD(0.0f, { return t->e->predict_csr(label, ng, nu, ni, index, value); })
}
int svdf_update_csr_batch(svdf_trainer *t, int num_row, const float *row_label, const int *row_ptr,
                          const unsigned *feat_index, const float *feat_value) {
    SVDF_GUARD(-1, { t->e->update_csr_batch(num_row, row_label, row_ptr, feat_index, feat_value); return 0; })
}
int svdf_predict_csr_batch(svdf_trainer *t, int num_row, const float *row_label, const int *row_ptr,
                           const unsigned *feat_index, const float *feat_value, float *out) {
    SVDF_GUARD(-1, { t->e->predict_csr_batch(num_row, row_label, row_ptr, feat_index, feat_value, out); return 0; })
}
int svdf_update_block(svdf_trainer *t, int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row,
                      const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value) {
    SVDF_GUARD(-1, { t->e->update_block(nfb, tag, ifb, vfb, num_row, row_label, row_ptr, feat_index, feat_value); return 0; })
}
int svdf_predict_block(svdf_trainer *t, int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row,
                       const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value, float *out) {
    SVDF_GUARD(-1, { t->e->predict_block(nfb, tag, ifb, vfb, num_row, row_label, row_ptr, feat_index, feat_value, out); return 0; })
}

svdf_dataset *svdf_dataset_from_csr(svdf_trainer *t, long num_row, const float *row_label, const int64_t *row_ptr,
                                    const unsigned *feat_index, const float *feat_value) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_csr(num_row, row_label, row_ptr, feat_index, feat_value);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_from_triples(svdf_trainer *t, long n, const unsigned *user, const unsigned *item, const float *label) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_triples(n, user, item, label);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_window_from_triples(svdf_trainer *t, long n, const unsigned *user, const unsigned *item, const float *label) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_window_from_triples(n, user, item, label);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_window_from_pairs(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item, const unsigned *neg_item) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_window_from_pairs(n, user, pos_item, neg_item);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_window_from_csr(svdf_trainer *t, long num_row, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                           const float *feat_value) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_window_from_csr(num_row, row_label, row_ptr, feat_index, feat_value);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_window_from_blocks(svdf_trainer *t, long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index,
                                              const float *fb_value, const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr,
                                              const unsigned *feat_index, const float *feat_value) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_window_from_blocks(num_block, extend_tag, fb_ptr, fb_index, fb_value, block_row_ptr, row_label, row_ptr, feat_index, feat_value);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
int svdf_ipc_setup(svdf_trainer *t, int rank, int world, int64_t wire_bytes, int64_t block_floats, unsigned char *handles_out) { SVDF_GUARD(-1, { t->e->ipc_setup(rank, world, wire_bytes, block_floats, handles_out); return 0; }) }
int svdf_ipc_connect(svdf_trainer *t, const unsigned char *all_handles) { SVDF_GUARD(-1, { t->e->ipc_connect(all_handles); return 0; }) }
int svdf_ipc_window_pack(svdf_trainer *t, svdf_dataset *ds, int half) { SVDF_GUARD(-1, { t->e->ipc_window_pack(ds ? ds->d : nullptr, half); return 0; }) }
int svdf_ipc_window_reduce(svdf_trainer *t, int half) { SVDF_GUARD(-1, { t->e->ipc_window_reduce(half); return 0; }) }
int svdf_ipc_window_apply(svdf_trainer *t, int half) { SVDF_GUARD(-1, { t->e->ipc_window_apply(half); return 0; }) }
int svdf_ipc_block_send(svdf_trainer *t, int dst_rank, int slot) { SVDF_GUARD(-1, { t->e->ipc_block_send(dst_rank, slot); return 0; }) }
int svdf_ipc_block_recv(svdf_trainer *t, int src_rank, int slot, unsigned seq) { SVDF_GUARD(-1, { t->e->ipc_block_recv(src_rank, slot, seq); return 0; }) }
int svdf_ipc_status(svdf_trainer *t) { SVDF_GUARD(-1, { return t->e->ipc_status(); }) }
int svdf_ipc_close(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->ipc_close(); return 0; }) }
int svdf_rccl_unique_id(unsigned char *out128) { SVDF_GUARD(-1, { svdf::rccl_unique_id(out128); return 0; }) }
int svdf_rccl_init(svdf_trainer *t, const unsigned char *id128, int rank, int world) { SVDF_GUARD(-1, { t->e->rccl_init(id128, rank, world); return 0; }) }
int svdf_rccl_window_allreduce(svdf_trainer *t, svdf_dataset *ds, int half) { SVDF_GUARD(-1, { t->e->rccl_window_allreduce(ds ? ds->d : nullptr, half); return 0; }) }
int svdf_rccl_block_handoff(svdf_trainer *t, int dst_rank, int src_rank, int slot, int in_block, int nblocks) { SVDF_GUARD(-1, { t->e->rccl_block_handoff(dst_rank, src_rank, slot, in_block, nblocks); return 0; }) }
int svdf_rccl_block_arrive(svdf_trainer *t, int slot) { SVDF_GUARD(-1, { t->e->rccl_block_arrive(slot); return 0; }) }
int64_t svdf_rccl_counter(svdf_trainer *t, int what) { SVDF_GUARD(-1, { return t->e->rccl_counter(what); }) }
int svdf_rccl_close(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->rccl_close(); return 0; }) }
int svdf_window_delta_pack(svdf_trainer *t, svdf_dataset *ds, void *dst, int half, int64_t *count) {
    SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->window_delta_pack(ds ? ds->d : nullptr, dst, half, count); return 0; })
}
int svdf_window_delta_apply_local(svdf_trainer *t, svdf_dataset *ds) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->window_delta_apply_local(ds ? ds->d : nullptr); return 0; }) }
int svdf_item_block_get(svdf_trainer *t, float *dst, int64_t *count) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_block_copy(dst, 0, count); return 0; }) }
int svdf_stratum_step(svdf_trainer *t, svdf_dataset *const *windows, int num_windows, int block, int nblocks, float *device_out) {
    SVDF_GUARD(-1, {
        t->e->per_rank_api();
        std::vector<svdf::Dataset *> d((size_t)(num_windows > 0 ? num_windows : 0));
        for (int w = 0; w < num_windows; w++) d[(size_t)w] = windows[w] ? windows[w]->d : nullptr;
        t->e->stratum_step(d.data(), num_windows, block, nblocks, device_out);
        return 0;
    })
}
int svdf_item_block_set_at(svdf_trainer *t, int block, int nblocks, const float *src) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_block_set_at(block, nblocks, src); return 0; }) }
int svdf_item_block_set(svdf_trainer *t, const float *src) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_block_copy(const_cast<float *>(src), 1, nullptr); return 0; }) }
int svdf_window_delta_apply(svdf_trainer *t, const void *src, int half) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->window_delta_apply(src, half); return 0; }) }
int svdf_debug_sort_labels(long n, const float *label, int *restated, int *library) {
    SVDF_GUARD(-1, {
        svdf::host_sort_by_label(label, n, restated);
        std::vector<int> ids((size_t)std::max<long>(n, 0));
        for (long j = 0; j < n; j++) ids[(size_t)j] = (int)j;
        std::sort(ids.begin(), ids.end(), [label](int a, int b) { return label[a] < label[b]; });
        for (long j = 0; j < n; j++) library[j] = ids[(size_t)j];
        return 0;
    })
}
int svdf_debug_sort_scores(long n, const float *score, int threads, int *parallel, int *library) {
    SVDF_GUARD(-1, {
        for (long j = 0; j < n; j++) parallel[j] = (int)j;
        svdf::host_parallel_sort_scores(score, parallel, n, threads);
        struct Entry { int iid; float score; bool operator<(const Entry &p) const { return score > p.score; } };   // apex_svd_base.h:617-624
        std::vector<Entry> e((size_t)std::max<long>(n, 0));
        for (long j = 0; j < n; j++) e[(size_t)j] = Entry{(int)j, score[j]};
        std::sort(e.begin(), e.end());
        for (long j = 0; j < n; j++) library[j] = e[(size_t)j].iid;
        return 0;
    })
}
svdf_dataset *svdf_dataset_from_pairs(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item, const unsigned *neg_item) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_pairs(n, user, pos_item, neg_item);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_from_blocks(svdf_trainer *t, long num_block, const int *extend_tag, const int64_t *fb_ptr,
                                       const unsigned *fb_index, const float *fb_value, const int64_t *block_row_ptr,
                                       const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                       const float *feat_value) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_blocks(num_block, extend_tag, fb_ptr, fb_index, fb_value, block_row_ptr, row_label, row_ptr,
                                                     feat_index, feat_value);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_from_buffer_file(svdf_trainer *t, const char *path, int user_group_format) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_buffer_file(path, user_group_format);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
svdf_dataset *svdf_dataset_from_rank_buffer_file(svdf_trainer *t, const char *path) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_rank_buffer_file(path);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
int svdf_rank_prefetch_buffer_file(svdf_trainer *t, const char *path) { SVDF_GUARD(-1, { t->e->rank_prefetch(path); return 0; }) }
int64_t svdf_rank_sample_buffer_file(svdf_trainer *t, const char *in_path, const char *out_path) {
    SVDF_GUARD(-1, { return (int64_t)t->e->rank_sample_buffer_file(in_path, out_path); })
}
void svdf_dataset_destroy(svdf_dataset *ds) {
    if (!ds) return;
    try { if (ds->d && ds->d->owner) ds->d->owner->synchronize(); } catch (...) {}
    delete ds->d;
    delete ds;
}
int svdf_train_dataset(svdf_trainer *t, svdf_dataset *ds) { SVDF_GUARD(-1, { t->e->train_dataset(ds->d); return 0; }) }
int svdf_predict_dataset(svdf_trainer *t, svdf_dataset *ds, float *out) { SVDF_GUARD(-1, { t->e->predict_dataset(ds->d, out); return 0; }) }
int64_t svdf_dataset_info(const svdf_dataset *ds, int what) {
    if (!ds || !ds->d) return -1;
    switch (what) {
    case 0: return ds->d->num_row;
    case 1: return ds->d->kind == 8 ? (int64_t)ds->d->wchild.size() : (int64_t)ds->d->sched.num_levels();   // kind 8: windows per pass
    case 2: return ds->d->sched.max_level_size;
    case 3: return ds->d->kind;
    case 4: return ds->d->algorithmic_bytes;
    case 5: return ds->d->num_units;
    case 6: return ds->d->num_simple_units;
    case 7: {   // FNV-1a over the host-resident schedule (level_ptr, level_mid, order): equal schedules <=> equal digests (tests)
        uint64_t h = 1469598103934665603ull;
        auto mix = [&h](uint64_t v) { for (int b = 0; b < 8; b++) { h ^= (v >> (8 * b)) & 0xFFu; h *= 1099511628211ull; } };
        for (long v : ds->d->sched.level_ptr) mix((uint64_t)v);
        for (long v : ds->d->sched.level_mid) mix((uint64_t)v);
        for (int v : ds->d->sched.order) mix((uint64_t)(unsigned)v);
        return (int64_t)(h >> 1);
    }
    case 8: return ds->d->kind == 8 && !ds->d->wchild.empty() ? (int64_t)ds->d->wchild[0]->kind : -1;
    case 9: return ds->d->rn_stage_state;   // runs data sets, operand staging: 0 not tried, 1 built, 2 refused (gate / no memory)
    case 10: return ds->d->rn_stage_bytes;  // ... bytes of the staging buffers
    case 11: return ds->d->kind == 10 ? ds->d->rn_wave_steps : -1;   // runs data sets, runs_wave_steps: sum over the pass kernel's aligned row sets of the longest run
    case 12: return ds->d->kind == 10 ? ds->d->rn_mixed_sets : -1;   // ... runs_mixed_sets: row sets whose runs differ in length
    case 13: return ds->d->kind == 10 ? ds->d->rn_order : -1;        // ... the in-level order the data set was built with (knob runs_order)
    default: return -1;
    }
}

int svdf_item_delta_begin(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_begin(); return 0; }) }
void *svdf_item_delta_buffer(svdf_trainer *t, int64_t *count) { SVDF_GUARD(nullptr, { t->e->per_rank_api(); return t->e->item_delta_buffer(count); }) }
int svdf_item_delta_apply(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_apply(); return 0; }) }
int svdf_item_delta_export(svdf_trainer *t, float *dst) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_copy(dst, nullptr); return 0; }) }
int svdf_item_delta_import(svdf_trainer *t, const float *src) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_copy(nullptr, src); return 0; }) }

int svdf_item_delta_into(svdf_trainer *t, float *dst, int64_t *count) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_into(dst, count); return 0; }) }
int svdf_item_delta_pack(svdf_trainer *t, void *dst, int half, int64_t *count) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_pack(dst, half, count); return 0; }) }
int svdf_item_delta_unpack(svdf_trainer *t, const void *src, int half, int refresh_snapshot) {
    SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_unpack(src, half, refresh_snapshot); return 0; })
}
int svdf_item_delta_select(svdf_trainer *t, int part, int nparts) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_select(part, nparts); return 0; }) }
int svdf_item_delta_apply_from(svdf_trainer *t, const float *src) { SVDF_GUARD(-1, { t->e->per_rank_api(); t->e->item_delta_apply_from(src); return 0; }) }
int svdf_set_stream(svdf_trainer *t, void *hip_stream) { SVDF_GUARD(-1, { t->e->set_stream((hipStream_t)hip_stream); return 0; }) }

int64_t svdf_get_view(svdf_trainer *t, int which, float *out, int64_t capacity) { SVDF_GUARD(-1, { return t->e->get_view(which, out, capacity); }) }
int64_t svdf_set_view(svdf_trainer *t, int which, const float *in, int64_t count) { SVDF_GUARD(-1, { return t->e->set_view(which, in, count); }) }
int svdf_view_shape(svdf_trainer *t, int which, int *rows, int *cols) { SVDF_GUARD(-1, { t->e->view_shape(which, rows, cols); return 0; }) }
void *svdf_stream(svdf_trainer *t) { return (void *)t->e->stream(); }
int svdf_synchronize(svdf_trainer *t) { SVDF_GUARD(-1, { t->e->synchronize(); return 0; }) }
int64_t svdf_counter(svdf_trainer *t, int what) { return t->e->counter(what); }
int svdf_set_knob(svdf_trainer *t, const char *name, long value) { SVDF_GUARD(-1, { return t->e->set_knob(name, value); }) }

int svdf_eval_dataset(svdf_trainer *t, svdf_dataset *ds, float scale_score, double *sum_sq_err, int64_t *count) {
    SVDF_GUARD(-1, { t->e->eval_dataset(ds->d, scale_score, sum_sq_err, count); return 0; })
}

/* ---- batch ranking evaluation on the live model ---- */
int svdf_rank_eval_positions(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item,
                             const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out) {
    SVDF_GUARD(-1, { t->e->rank_eval_positions(num_section, user, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out); return 0; })
}
int svdf_rank_eval_metrics(long num_section, const int64_t *sec_ptr, const int *position, const int *ranked, const int *nan, int num_at,
                           const int *at, svdf_rank_metrics *out) {
    SVDF_GUARD(-1, { svdf::rank_eval_metrics(num_section, sec_ptr, position, ranked, nan, num_at, at, out); return 0; })
}
int svdf_rank_eval(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item,
                   const int64_t *ban_ptr, const unsigned *ban_item, int num_at, const int *at, svdf_rank_metrics *out) {
    SVDF_GUARD(-1, {
        const size_t S = (size_t)std::max<long>(num_section, 0), np = S && pos_ptr ? (size_t)std::max<int64_t>(pos_ptr[S], 0) : 0;
        std::vector<int> position(np + 1), tied(np + 1), ranked(S + 1), nan(S + 1);
        t->e->rank_eval_positions(num_section, user, pos_ptr, pos_item, ban_ptr, ban_item, position.data(), tied.data(), ranked.data(), nan.data());
        svdf::rank_eval_metrics(num_section, pos_ptr, position.data(), ranked.data(), nan.data(), num_at, at, out);
        return 0;
    })
}
int svdf_rank_topn(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n,
                   int *item_out, float *score_out, int *count_out, int *nan_out) {
    SVDF_GUARD(-1, { t->e->rank_topn(num_section, user, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out); return 0; })
}
/* ... for sections with feedback lists (user-group trainers) */
int svdf_rank_eval_positions_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index,
                                const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                                const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out) {
    SVDF_GUARD(-1, {
        t->e->rank_eval_positions_fb(num_section, user, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out, nan_out);
        return 0;
    })
}
int svdf_rank_eval_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                      const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_at, const int *at,
                      svdf_rank_metrics *out) {
    SVDF_GUARD(-1, {
        const size_t S = (size_t)std::max<long>(num_section, 0), np = S && pos_ptr ? (size_t)std::max<int64_t>(pos_ptr[S], 0) : 0;
        std::vector<int> position(np + 1), tied(np + 1), ranked(S + 1), nan(S + 1);
        t->e->rank_eval_positions_fb(num_section, user, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position.data(), tied.data(),
                                     ranked.data(), nan.data());
        svdf::rank_eval_metrics(num_section, pos_ptr, position.data(), ranked.data(), nan.data(), num_at, at, out);
        return 0;
    })
}
/* similar-item lists on the live model */
int svdf_item_topn(svdf_trainer *t, long num_section, const unsigned *item, int metric, const int64_t *ban_ptr, const unsigned *ban_item, int top_n,
                   int *item_out, float *score_out, int *count_out, int *nan_out) {
    SVDF_GUARD(-1, { t->e->item_topn(num_section, item, metric, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out); return 0; })
}
int svdf_item_unit_rows(long num_row, int num_factor, const float *rows, float *out) {
    SVDF_GUARD(-1, { svdf::item_unit_rows(num_row, num_factor, rows, out); return 0; })
}
int svdf_rank_topn_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                      const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    SVDF_GUARD(-1, { t->e->rank_topn_fb(num_section, user, fb_ptr, fb_index, fb_value, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out); return 0; })
}
/* ... for sections that bring a USER line, on trainers with or without side tables */
int svdf_rank_eval_positions_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                                   const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                   const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out,
                                   int *ranked_out, int *nan_out) {
    SVDF_GUARD(-1, {
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_eval_positions_lines(num_section, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position_out, tied_out, ranked_out,
                                        nan_out);
        return 0;
    })
}
int svdf_rank_eval_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value, const int64_t *fb_ptr,
                         const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                         const unsigned *ban_item, int num_at, const int *at, svdf_rank_metrics *out) {
    SVDF_GUARD(-1, {
        const size_t S = (size_t)std::max<long>(num_section, 0), np = S && pos_ptr ? (size_t)std::max<int64_t>(pos_ptr[S], 0) : 0;
        std::vector<int> position(np + 1), tied(np + 1), ranked(S + 1), nan(S + 1);
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_eval_positions_lines(num_section, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, position.data(), tied.data(),
                                        ranked.data(), nan.data());
        svdf::rank_eval_metrics(num_section, pos_ptr, position.data(), ranked.data(), nan.data(), num_at, at, out);
        return 0;
    })
}
int svdf_rank_topn_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value, const int64_t *fb_ptr,
                         const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out,
                         float *score_out, int *count_out, int *nan_out) {
    SVDF_GUARD(-1, {
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_topn_lines(num_section, U, fb_ptr, fb_index, fb_value, ban_ptr, ban_item, top_n, item_out, score_out, count_out, nan_out);
        return 0;
    })
}
/* ... and over per-section candidate lists in place of the catalogue minus bans */
int svdf_rank_eval_positions_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                                  const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                  const unsigned *pos_item, const int64_t *cand_ptr, const unsigned *cand_item, int *position_out, int *tied_out,
                                  int *ranked_out, int *nan_out) {
    SVDF_GUARD(-1, {
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_cand("rank_eval", num_section, user, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, cand_ptr, cand_item, 0, position_out, tied_out,
                        ranked_out, nullptr, nullptr, nullptr, nan_out);
        return 0;
    })
}
int svdf_rank_eval_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                        const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item,
                        const int64_t *cand_ptr, const unsigned *cand_item, int num_at, const int *at, svdf_rank_metrics *out) {
    SVDF_GUARD(-1, {
        const size_t S = (size_t)std::max<long>(num_section, 0), np = S && pos_ptr ? (size_t)std::max<int64_t>(pos_ptr[S], 0) : 0;
        std::vector<int> position(np + 1), tied(np + 1), ranked(S + 1), nan(S + 1);
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_cand("rank_eval", num_section, user, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, cand_ptr, cand_item, 0, position.data(),
                        tied.data(), ranked.data(), nullptr, nullptr, nullptr, nan.data());
        svdf::rank_eval_metrics(num_section, pos_ptr, position.data(), ranked.data(), nan.data(), num_at, at, out);
        return 0;
    })
}
int svdf_rank_topn_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                        const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *cand_ptr, const unsigned *cand_item,
                        int top_n, int *item_out, float *score_out, int *count_out, int *nan_out) {
    SVDF_GUARD(-1, {
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_cand("rank_topn", num_section, user, U, fb_ptr, fb_index, fb_value, nullptr, nullptr, cand_ptr, cand_item, top_n, nullptr, nullptr,
                        nullptr, item_out, score_out, count_out, nan_out);
        return 0;
    })
}

/* ... and against negatives drawn on the device from (seed, section, what the section excludes) */
int svdf_rank_negatives(long num_section, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                        long num_item, int num_neg, uint64_t seed, int *neg_out) {
    SVDF_GUARD(-1, { svdf::rank_negs_host(num_section, pos_ptr, pos_item, ban_ptr, ban_item, num_item, num_neg, seed, neg_out); return 0; })
}
int svdf_rank_eval_positions_sampled(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                                     const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                     const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg,
                                     uint64_t seed, int *position_out, int *tied_out, int *ranked_out, int *nan_out, int *neg_out) {
    SVDF_GUARD(-1, {
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_negs(num_section, user, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, seed, position_out, tied_out,
                        ranked_out, nan_out, neg_out);
        return 0;
    })
}
int svdf_rank_eval_sampled(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                           const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                           const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg, uint64_t seed, int num_at,
                           const int *at, svdf_rank_metrics *out) {
    SVDF_GUARD(-1, {
        const size_t S = (size_t)std::max<long>(num_section, 0), np = S && pos_ptr ? (size_t)std::max<int64_t>(pos_ptr[S], 0) : 0;
        std::vector<int> position(np + 1), tied(np + 1), ranked(S + 1), nan(S + 1);
        svdf::RankLines U;
        U.ptr = ul_ptr; U.index = ul_index; U.value = ul_value;
        t->e->rank_negs(num_section, user, U, fb_ptr, fb_index, fb_value, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, seed, position.data(),
                        tied.data(), ranked.data(), nan.data(), nullptr);
        svdf::rank_eval_metrics(num_section, pos_ptr, position.data(), ranked.data(), nan.data(), num_at, at, out);
        return 0;
    })
}

/* ---- passes of rank pairs from positives only: the negatives drawn on the device ---- */
svdf_pair_source *svdf_pair_source_create(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item) {
    SVDF_GUARD(nullptr, {
        svdf::PairSource *s = t->e->pair_source_create(n, user, pos_item);
        svdf_pair_source *h = new svdf_pair_source();
        h->s = s;
        return h;
    })
}
void svdf_pair_source_destroy(svdf_pair_source *s) {
    if (!s) return;
    try { delete s->s; } catch (...) {}
    delete s;
}
svdf_dataset *svdf_dataset_from_pair_source(svdf_trainer *t, svdf_pair_source *s, int num_neg, uint64_t seed) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_pair_source(s ? s->s : nullptr, num_neg, seed);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
int svdf_pair_source_draw(svdf_trainer *t, svdf_pair_source *s, int num_neg, uint64_t seed, unsigned *neg_out) {
    SVDF_GUARD(-1, { t->e->pair_source_draw(s ? s->s : nullptr, num_neg, seed, neg_out); return 0; })
}
int svdf_pair_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, uint64_t seed,
                        unsigned *neg_out) {
    SVDF_GUARD(-1, { svdf::pair_src_negatives(num_user, num_item, n, user, pos_item, num_neg, seed, neg_out); return 0; })
}
/* ... and the hard pass: the best of num_cand candidates by live score */
svdf_dataset *svdf_dataset_from_pair_source_hard(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed) {
    SVDF_GUARD(nullptr, {
        if (num_cand == 0) svdf::fail("pair_source: num_cand must be between 1 and 256");   // (0 selects the plain pass inside the engine)
        svdf::Dataset *d = t->e->dataset_from_pair_source(s ? s->s : nullptr, num_neg, seed, num_cand);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
int svdf_pair_source_draw_hard(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed, unsigned *neg_out, float *score_out) {
    SVDF_GUARD(-1, {
        if (num_cand == 0) svdf::fail("pair_source: num_cand must be between 1 and 256");
        t->e->pair_source_draw(s ? s->s : nullptr, num_neg, seed, neg_out, num_cand, score_out);
        return 0;
    })
}
int svdf_pair_hard_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, int num_cand,
                             uint64_t seed, int num_factor, const float *W_user, const float *W_item, const float *i_bias, unsigned *neg_out,
                             float *score_out) {
    SVDF_GUARD(-1, {
        svdf::pair_hard_negatives(num_user, num_item, n, user, pos_item, num_neg, num_cand, seed, num_factor, W_user, W_item, i_bias, neg_out, score_out);
        return 0;
    })
}
/* ... and the shuffled pass: the rows in the order sigma of an order_seed; num_cand = 0 is the plain pass */
svdf_dataset *svdf_dataset_from_pair_source_shuffled(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed, uint64_t order_seed) {
    SVDF_GUARD(nullptr, {
        svdf::Dataset *d = t->e->dataset_from_pair_source(s ? s->s : nullptr, num_neg, seed, num_cand, &order_seed);
        t->e->note_dataset(d);
        svdf_dataset *h = new svdf_dataset();
        h->d = d;
        return h;
    })
}
int svdf_pair_source_draw_shuffled(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed, uint64_t order_seed, unsigned *user_out,
                                   unsigned *pos_out, unsigned *neg_out, float *score_out) {
    SVDF_GUARD(-1, {
        t->e->pair_source_draw(s ? s->s : nullptr, num_neg, seed, neg_out, num_cand, num_cand > 0 ? score_out : nullptr, &order_seed, user_out, pos_out);
        return 0;
    })
}
int svdf_pair_order(long n, uint64_t order_seed, unsigned *sigma_out) {
    SVDF_GUARD(-1, { svdf::pair_order_host(n, order_seed, sigma_out); return 0; })
}
/* ... and item-weighted negatives, plain and hard */
svdf_pair_source *svdf_pair_source_create_weighted(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight) {
    SVDF_GUARD(nullptr, {
        svdf::PairSource *s = t->e->pair_source_create(n, user, pos_item, item_weight);
        svdf_pair_source *h = new svdf_pair_source();
        h->s = s;
        return h;
    })
}
int svdf_pair_negatives_weighted(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight,
                                 int num_neg, uint64_t seed, unsigned *neg_out) {
    SVDF_GUARD(-1, {
        if (!item_weight) svdf::pair_src_negatives(num_user, num_item, n, user, pos_item, num_neg, seed, neg_out);
        else svdf::pair_weight_negatives(num_user, num_item, n, user, pos_item, item_weight, num_neg, seed, neg_out);
        return 0;
    })
}
int svdf_pair_hard_negatives_weighted(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight,
                                      int num_neg, int num_cand, uint64_t seed, int num_factor, const float *W_user, const float *W_item,
                                      const float *i_bias, unsigned *neg_out, float *score_out) {
    SVDF_GUARD(-1, {
        svdf::pair_hard_negatives(num_user, num_item, n, user, pos_item, num_neg, num_cand, seed, num_factor, W_user, W_item, i_bias, neg_out, score_out,
                                  item_weight);
        return 0;
    })
}

/* ---- ISVDRanker ---- */
svdf_ranker *svdf_ranker_create(uint8_t format_type, uint8_t active_type, uint8_t extend_type, uint8_t variant_type, int device) {
    SVDF_GUARD(nullptr, {
        svdf::TypeParam tp{format_type, active_type, extend_type, variant_type};
        svdf_ranker *h = new svdf_ranker();
        h->r = nullptr;
        try { h->r = new svdf::Ranker(tp, device); } catch (...) { delete h; throw; }
        return h;
    })
}
void svdf_ranker_destroy(svdf_ranker *r) {
    if (!r) return;
    try { delete r->r; } catch (...) {}
    delete r;
}
int svdf_ranker_set_param(svdf_ranker *r, const char *name, const char *val) { SVDF_GUARD(-1, { r->r->set_param(name, val); return 0; }) }
int svdf_ranker_load_model(svdf_ranker *r, FILE *fi) { SVDF_GUARD(-1, { r->r->load_model(fi); return 0; }) }
int svdf_ranker_init(svdf_ranker *r, int num_item_set) { SVDF_GUARD(-1, { r->r->init_ranker(num_item_set); return 0; }) }
int64_t svdf_ranker_process_csr(svdf_ranker *r, float label, int ng, int nu, int ni, const unsigned *index, const float *value, int *out,
                                int64_t capacity) {
    SVDF_GUARD(-1, { return (int64_t)r->r->process(label, ng, nu, ni, index, value, out, (long)capacity); })
}
int64_t svdf_ranker_process_rows(svdf_ranker *r, int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index,
                                 const float *feat_value, int *out, int64_t capacity) {
    SVDF_GUARD(-1, { return (int64_t)r->r->process_rows(num_row, row_label, row_ptr, feat_index, feat_value, out, (long)capacity); })
}
int64_t svdf_ranker_process_block(svdf_ranker *r, int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row, const float *row_label,
                                  const int *row_ptr, const unsigned *feat_index, const float *feat_value, int *out, int64_t capacity) {
    SVDF_GUARD(-1, { return (int64_t)r->r->process_block(nfb, tag, ifb, vfb, num_row, row_label, row_ptr, feat_index, feat_value, out, (long)capacity); })
}
int64_t svdf_ranker_counter(svdf_ranker *r, int what) { return r->r->counter(what); }

int svdf_rand_peek(long n, int *out) { SVDF_GUARD(-1, { svdf::libc_rand_peek(n, out); return 0; }) }
int svdf_rand_skip(long n) { SVDF_GUARD(-1, { svdf::libc_rand_skip(n); return 0; }) }

int svdf_device_expf(const float *in, unsigned first_bits, unsigned step_bits, float *out, long n) {
    SVDF_GUARD(-1, { return svdf::device_expf(in, first_bits, step_bits, out, n); })
}

// the launch choice of the level kernels exposed for tests (tests/test_level_geometry.py): Engine::level_geometry
int svdf_level_geometry(svdf_trainer *t, int launcher, long n, int max_nu, int max_ni, int unit_values, int has_globals, long *out) {
    SVDF_GUARD(-1, { t->e->level_geometry(launcher, n, max_nu, max_ni, unit_values, has_globals, out); return 0; })
}
// the launch geometry of the live-model ranking calls exposed for tests (tests/test_rank_geometry.py): Engine::rank_geometry
int svdf_rank_geometry(svdf_trainer *t, int kind, long units, int top_n, const int64_t *pos_ptr, long *out) {
    SVDF_GUARD(-1, { t->e->rank_geometry(kind, units, top_n, pos_ptr, out); return 0; })
}
// the map of a weighted pair source exposed for tests (tests/test_pair_weight.py): svdf_pairweight_lists.h on the host (t == NULL), the same
// function in one small launch on the device (Engine::pair_weight_lookup)
int svdf_pair_weight_lookup(svdf_trainer *t, long num_item, const unsigned *item_weight, int form, long nx, const uint64_t *x, unsigned *id_out) {
    SVDF_GUARD(-1, {
        if (t) { t->e->pair_weight_lookup(num_item, item_weight, form, nx, x, id_out); return 0; }
        if (form < 0 || form > 2 || nx < 0 || (nx > 0 && (!x || !id_out))) svdf::fail("pair_weight_lookup: bad arguments");
        svdf::PairWeightLists Wt;
        svdf::pair_weight_build(num_item, item_weight, Wt);
        svdf::pair_weight_lookup_host(Wt.view(), form == 0 ? svdf::pair_weight_form(num_item, 0) : form, nx, x, id_out);
        return 0;
    })
}

// the window rule exposed for CPU tests (tests/test_window_rule.py): svdf_wseq_rule.h, the functions the data-set builders call
long svdf_window_rule(int route, const svdf_window_rule_in *in) {
    SVDF_GUARD(-1, {
        if (!in || route < 0 || route > 2) svdf::fail("svdf_window_rule: bad arguments");
        svdf::WseqKnobs K;
        K.per_target = in->per_target; K.per_target_max = in->per_target_max; K.per_target_fb = in->per_target_fb;
        K.per_target_shared = in->per_target_shared; K.per_target_child = in->per_target_child; K.window = in->window;
        const svdf::WseqLane shared_lane{in->shared_sub, in->shared_cap}, item_lane{in->item_sub, in->item_cap};
        svdf::WseqCounts C;
        C.ci.assign(in->item_count, in->item_count + in->num_item);
        if (route == 0) return svdf::wseq_rule_columns(K, in->n, C.ci, item_lane);
        C.cg.assign(in->global_count, in->global_count + in->num_global);
        C.cs.assign(in->shared_count, in->shared_count + in->num_shared);
        if (in->item_child) C.ichild.assign(in->item_child, in->item_child + in->num_item);
        if (in->shared_child) C.uchild.assign(in->shared_child, in->shared_child + in->num_shared);
        if (route == 1) return svdf::wseq_rule_csr(K, in->n, C, shared_lane, item_lane);
        return svdf::wseq_rule_blocks(K, in->n, in->num_block, C, std::vector<double>(in->fb_mass, in->fb_mass + in->num_fb), shared_lane, item_lane);
    })
}
long svdf_window_rule_as_cut(long W, long n, int ncol, const unsigned *const *cols, long num_id, double target, long cap, int sub, double slack,
                             int rounds) {
    SVDF_GUARD(-1, {
        if (W < 1 || n < 0 || ncol < 1 || !cols || num_id < 0) svdf::fail("svdf_window_rule_as_cut: bad arguments");
        for (int c = 0; c < ncol; c++)
            for (long r = 0; r < n; r++) if ((long)cols[c][r] >= num_id) svdf::fail("svdf_window_rule_as_cut: an id is out of range");
        return svdf::wseq_windows_actual_columns(W, n, svdf::WseqClass{num_id, target, cap, sub}, std::vector<const unsigned *>(cols, cols + ncol), slack, rounds, true);
    })
}
int svdf_window_block_cuts(long num_block, const int *extend_tag, long W, long *cut_out) {
    SVDF_GUARD(-1, {
        if (num_block < 0 || W < 1 || !cut_out) svdf::fail("svdf_window_block_cuts: bad arguments");
        const std::vector<long> cut = svdf::wseq_block_cuts(num_block, extend_tag, W);
        std::copy(cut.begin(), cut.end(), cut_out);
        return 0;
    })
}

// host-side scheduler exposed for CPU tests (tests/test_scheduler.py): levels for a CSR stream over
// `num_res` resources where instance r touches resources res[res_ptr[r]..res_ptr[r+1]).
int svdf_schedule_resources(long n, const int64_t *res_ptr, const unsigned *res, long num_res, int *order_out,
                            int64_t *level_ptr_out, long level_cap) {
    SVDF_GUARD(-1, {
        std::vector<int> last((size_t)num_res, 0), levels((size_t)n);
        for (long r = 0; r < n; r++) {
            int l = 0;
            for (int64_t j = res_ptr[r]; j < res_ptr[r + 1]; j++) l = std::max(l, last[res[j]]);
            l += 1;
            for (int64_t j = res_ptr[r]; j < res_ptr[r + 1]; j++) last[res[j]] = l;
            levels[(size_t)r] = l;
        }
        svdf::Schedule s;
        svdf::build_schedule(levels, 0, s);
        if ((long)s.num_levels() + 1 > level_cap) return -2;
        for (long r = 0; r < n; r++) order_out[r] = s.order[(size_t)r];
        for (size_t l = 0; l <= s.num_levels(); l++) level_ptr_out[l] = s.level_ptr[l];
        return (int)s.num_levels();
    })
}

}  // extern "C"

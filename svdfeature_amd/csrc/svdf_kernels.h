// svdf_kernels.h -- launch wrappers of the gfx950 kernels (svdf_k_*.hip)
#ifndef SVDF_KERNELS_H_
#define SVDF_KERNELS_H_

#include <hip/hip_runtime.h>

#include <type_traits>
#include <vector>

#include "svdf_types.h"
#include "svdf_level_geometry.h"
#include "svdf_pairweight_lists.h"
#include "svdf_pairorder_lists.h"

namespace svdf {

// lanes of a wave that own one factor row (one float4 each): next power of two >= ceil(k/4)
int lanes_per_instance(int k);
int max_supported_factor();
int max_fast_path_factor();   // widest row of the register-tiled kernels (k_basicmf, k_fused, simple SVD++ units)

// every launch below processes ONE conflict-free batch [begin,end) on stream st
void launch_basicmf(const DevParams &P, const BasicSchedule &S, long begin, long end, int groups_per_wave, int block_threads, hipStream_t st);
bool launch_basicmf_chain(const DevParams &P, const BasicSchedule &S, const long *d_level_ptr, long l0, long l1, hipStream_t st);
// few-row fused kernel: instances with <= max_nu (1|2) user ids and <= max_ni (1|2) item ids
void launch_fused(const DevParams &P, const FusedSchedule &S, int max_nu, int max_ni, long begin, long end, int groups_per_wave,
                  int block_threads, hipStream_t st);
// the same step specialised for data sets without global features under L2 decay without ranges / relaxed ids (svdf_k_fewrow.hip)
bool fewrow_fast_applies(const DevParams &P, const FusedSchedule &S);
bool launch_fewrow_chain(const DevParams &P, const FusedSchedule &S, int max_nu, int max_ni, const long *d_level_ptr, long l0, long l1, hipStream_t st);
bool fewrow_gslots_applies(const DevParams &P, const FusedSchedule &S, int max_nu, int max_ni, bool dense_slots);
void launch_fewrow_gslots(const DevParams &P, const FusedSchedule &S, long begin, long end, hipStream_t st);
void launch_fewrow_fast(const DevParams &P, const FusedSchedule &S, int max_nu, int max_ni, long begin, long end, int block_threads, hipStream_t st);
void launch_predict_fused(const DevParams &P, const FusedSchedule &S, int max_nu, int max_ni, long n, float *out, hipStream_t st);
// counter_base: the reference's sample_counter at the first instance of D (row r runs with counter_base + r); only the
// lazy decay modes read it
void launch_general(const DevParams &P, const DevCSR &D, const int *order, long begin, long end, unsigned counter_base, hipStream_t st);
void launch_svdpp(const DevParams &P, const DevCSR &D, const DevUnit *units, const unsigned *fb_index, const float *fb_value,
                  const int *order, long begin, long end, unsigned counter_base, hipStream_t st);
// units flagged UNIT_SIMPLE (num_factor <= 256): one wave per user, see k_svdpp_wave
void launch_svdpp_wave(const DevParams &P, const DevCSR &D, const DevUnit *units, const unsigned *fb_index, const float *fb_value,
                       const int *order, const DevUnitX *xunits, long begin, long end, hipStream_t st);
// extend_type 2 (multi-level implicit feedback): units = block ranges of blks[]; predict_out != nullptr scores instead of training
void launch_imfb(const DevParams &P, const DevCSR &D, const DevUnit *units, const DevBlk *blks, const unsigned *fb_index, const float *fb_value,
                 const int *order, long begin, long end, unsigned counter_base, float *predict_out, hipStream_t st);
// read-only scoring
void launch_predict(const DevParams &P, const DevCSR &D, long n, float *out, hipStream_t st);
void launch_predict_basic(const DevParams &P, const BasicSchedule &S, long n, float *out, hipStream_t st);
void launch_svdpp_predict(const DevParams &P, const DevCSR &D, const DevUnit *units, const unsigned *fb_index, const float *fb_value,
                          long nunit, float *out, hipStream_t st);
// multi-GPU item-side delta over n floats
void launch_delta_pack(const DeltaRanges &R, const float *snap, void *dst, int half, hipStream_t st);
void launch_delta_unpack(const DeltaRanges &R, float *snap, const void *src, int half, int refresh, hipStream_t st);
// window-minibatch step (svdf_k_window.hip): user walk with the item side read-only, per-item sum of the contributions into the wire
// buffer (item range [lo, hi) + nglobal zeros), and replicated ranges += all-reduced wire buffer
bool window_slots_applies(const DevParams &P, const WindowSchedule &S);
void launch_window_apply(const DevParams &P, const WindowSchedule &S, long num_item, float *w_item, float *i_bias, hipStream_t st);   // a window WITH hot items: ordered sub-steps of the hot ones beside the in-place sums of the others, one launch
void launch_window_apply_pairs(const DevParams &P, const WindowSchedule &S, long num_item, hipStream_t st);   // rank pairs, a window WITH hot items: their ordered sub-steps (the model is not written; a hot row's final value goes to its first slot)
void launch_window_pair_sums(const WindowSchedule &S, int pitch, int k, long num_item, float *w_item, float *i_bias, hipStream_t st);   // ... then hot rows moved in, the others' slots summed in place
void launch_window_users(const DevParams &P, const WindowSchedule &S, int slots, int groups_per_wave, hipStream_t st);
void launch_window_items(const WindowSchedule &S, int pitch, int k, long lo, long hi, long nglobal, void *dst, int half, hipStream_t st, long nslots = -1);
void launch_delta_addto(const DeltaRanges &R, const void *src, int half, hipStream_t st);
void launch_window_items_local(const WindowSchedule &S, int pitch, int k, long lo, long hi, float *w_item, float *i_bias, hipStream_t st, long nslots = -1);   // nslots: contributions in the window (sparse windows take k_window_items_sparse)
void launch_ranges_copy(const DeltaRanges &R, float *buf, int set, hipStream_t st);
// the same step for user units: user-group (SVD++) blocks, rows with global features (svdf_k_wunit.hip)
// returns the form that ran: 0 the general or slot kernel, 1 the wave form with the segments' shared user rows in registers, 2 the plain wave form
int launch_wunit_walk(const DevParams &P, const WUnitSchedule &S, bool feedback, int fast, hipStream_t st, bool shared_uniform = false);
bool wunit_wave_applies(const DevParams &P, const WUnitSchedule &S, bool feedback);   // svdf_k_wave.hip: one wave per user unit (SVD++ shape)
void launch_wunit_wave(const DevParams &P, const WUnitSchedule &S, hipStream_t st, bool shared = false);
void launch_wunit_apply_shared(const DevParams &P, const WUnitSchedule &S, hipStream_t st, bool feedback = false);   // hot shared user rows in ordered sub-steps, between the walk and the in-place sums
void launch_wunit_apply_item(const DevParams &P, const WUnitSchedule &S, long nitem_hot, hipStream_t st, bool feedback = false);   // hot item rows (S.hot[S.nhot .. + nitem_hot)) likewise; writes no model row either, so its order against the launch above is free
void launch_wunit_sum(const DevParams &P, const WUnitSchedule &S, void *dst, int half, hipStream_t st);   // dst == nullptr: add to the model in place
// cross-process direct exchange (svdf_ipc.cpp): sequence flags in IPC-mapped device memory
void launch_ipc_signal(unsigned *const *pages, int n, int phase, int me, unsigned seq, const unsigned *err, hipStream_t st);
void launch_ipc_wait(unsigned *page, int phase, int n, unsigned seq, unsigned *err, unsigned long long spin_limit, hipStream_t st);
void launch_ipc_copy(float *dst, const float *src, long n, const unsigned *err, hipStream_t st);
void launch_window_user_column(const WinUser *urec, int nusers, unsigned *user_out, hipStream_t st);
// read-only scoring of window data sets.  pos == nullptr: out[r] in regrouped order, else out[pos[r]] (file order)
void launch_window_predict_pairs(const DevParams &P, const WindowSchedule &S, const unsigned *user_col, long n, const int *pos, float *out, hipStream_t st);
void launch_wunit_score_columns(const WUnitSchedule &S, unsigned *user_col, int *seg_col, hipStream_t st);   // the user and segment of every regrouped row
void launch_wunit_score_prepare(const DevParams &P, const WUnitSchedule &S, long nseg, float *fbvec, float *fbbias, hipStream_t st);   // prepare_ufeedback per segment
void launch_wunit_score(const DevParams &P, const WUnitSchedule &S, bool feedback, const unsigned *user_col, const int *seg_col, const float *fbvec,
                        const float *fbbias, long nrow, const int *pos, float *out, hipStream_t st);
void launch_pairs_prepare(long n, const unsigned *pos, const unsigned *neg, unsigned *lo, unsigned *hi, float *vlo, float *vhi, float *ones,
                          unsigned *flag, hipStream_t st);
void launch_delta_sum(const void *const *srcs, int n, void *dst, long total, int half, hipStream_t st);   // up to 16 buffers
// rank d's share of the direct exchange: elements [begin, end) of every buffer <- their sum over the n buffers (rank order, fp32)
void launch_delta_reduce_gather(void *const *bufs, int n, long begin, long end, int half, hipStream_t st, const unsigned *err = nullptr);
void launch_rows_strided_copy(float *dst, long dst_first, long dst_stride, const float *src, long src_first, long src_stride, long nrows, int width,
                              hipStream_t st);
void launch_delta_sub(const float *cur, const float *snap, float *delta, long n, hipStream_t st);
void launch_delta_add(float *cur, const float *snap, const float *delta, long n, hipStream_t st);
// ---- ranker (svdf_k_rank.hip): SVDFeatureRanker's prepare_ifactor / proc_user / proc_spec / proc_rank, and the evaluator's sum
void launch_rank_items(const DevParams &P, const DevCSR &D, long first, long n, float *ifactors, float *ibias, hipStream_t st);
void launch_rank_feedback(const DevParams &P, const unsigned *fidx, const float *fval, int nfb, float *fb_out, hipStream_t st);
struct RankSection { int nu, npos, nprev, nnew; };   // words staged per ranker section: uidx[nu] uval[nu] pos[npos] prev[nprev] new_idx[nnew] new_tag[nnew]
void launch_rank_user(const DevParams &P, const unsigned *stage, const RankSection &S, const float *fb_in, float *tu_out, signed char *tag, int *cnt,
                      unsigned *flag, long cap, const float *ifT, const float *ibias, float *pos_score, unsigned *zero_words, int nzero, hipStream_t st);
void launch_rank_spec(const DevParams &P, const DevCSR &D, long n, const int *spec_idx, const float *tu, float *item_score, hipStream_t st);
void launch_rank_transpose(const DevParams &P, long first, long n, long cap, const float *ifactors, float *ifT, hipStream_t st);
// what the scoring pass does besides the scores: 1 = count the positives' rank positions, 2 = emit the top_k sort keys
struct RankFused { int mode; const int *pos_item; const float *pos_score; int npos; int *greater, *ties; unsigned *keys, *vals, *flag, *hist1; };
void launch_rank_score(const DevParams &P, long n, long cap, const float *tu, const float *ifT, const float *ibias, const signed char *tag,
                       float *item_score, int fresh, const RankFused &F, hipStream_t st);
// a tile of user sections sharing one pass over the candidate matrix (no special samples): per section u the staged words at off[u] are
// uidx[nu] uval[nu] pos[npos] ban[nban]; its counters / positive scores start at entry pos0[u].  32 = the bits of a ban word.
#define RANK_TILE 32
struct RankTile { int nsec; int off[RANK_TILE], nu[RANK_TILE], npos[RANK_TILE], nban[RANK_TILE], pos0[RANK_TILE]; };
// tuT: the tile's user factors chunk-major, RANK_TILE * pitch floats (written here, read as scalars by the scoring pass)
void launch_rank_tile_open(const DevParams &P, const unsigned *stage, const RankTile &T, const float *fb_in, float *tuT, unsigned *banmask,
                           const unsigned *prev_ban, int nprev, int *cnt, unsigned *flag, long cap, const float *ifT, const float *ibias, float *pos_score,
                           unsigned *zero_words, long nzero, hipStream_t st);
// mode 0: out[u * cap + i] = score bits of the ranked candidates + the positives' counters; mode 1: out = sort keys of every candidate,
// wmin[u * rank_tile_minima(n) + wave] = per-wave minimum keys
void launch_rank_score_tile(const DevParams &P, long n, long cap, const float *tuT, const float *ifT, const float *ibias, const unsigned *banmask, unsigned *out,
                            const unsigned *stage, const RankTile &T, const float *pos_score, int *cnt, int mode, unsigned *wmin, unsigned *flag, hipStream_t st);
struct RselSecs { unsigned K1[RANK_TILE]; };
long rank_tile_minima(long n);
bool rank_tile_select_applies(long n, long cap, long K1max);
// top_k of every section of a tile from its keys and wave minima: out + u * out_stride = K1[u] keys, K1[u] candidates, flag word
void launch_rank_tile_select(long n, long cap, int nsec, const unsigned *keys, const unsigned *wmin, const RselSecs &Ks, unsigned *out, long out_stride,
                             const unsigned *flag, hipStream_t st);
void launch_rank_select_tile(long n, long cap, int nsec, const unsigned *keys, const RselSecs &Ks, unsigned *work, unsigned *ck, unsigned *cv, unsigned *out,
                             long out_stride, unsigned *flag, hipStream_t st);
void launch_rank_positions(long n, const float *score, const signed char *tag, const int *pos_item, int npos, int *greater, int *ties, hipStream_t st);
// radix selection of the K1 smallest (key, value) pairs, ascending (svdf_k_rank.hip): work = rank_select_work_words() words
// (zeroed by k_rank_user, first histogram filled by the scoring pass: RankFused::hist1 = work), ck / cv = rank_select_cap()
// words each, K1 <= rank_select_cap() / 2; out = K1 keys, K1 values, flag word (| 2 when too many keys tie at the threshold)
long rank_select_work_words();
long rank_select_cap();
void launch_rank_select(long n, const unsigned *keys, const unsigned *vals, unsigned K1, unsigned *work, unsigned *ck, unsigned *cv, unsigned *out,
                        const unsigned *flag, hipStream_t st);
// ascending radix sort of (key, value) pairs (svdf_k_sched.hip, rocPRIM); tmp is grown as needed
long device_exclusive_scan_u32(const unsigned *in, unsigned *out, long n, void **tmp, size_t *tmp_bytes, hipStream_t st);
// runs of an item's consecutive ratings as schedule units (svdf_k_runs.hip)
void launch_runs_check(const unsigned *user, const unsigned *item, long n, unsigned nu, unsigned ni, unsigned *flag, hipStream_t st);
void launch_runs_prev(const unsigned *keys, const unsigned *pos, long n, unsigned *prev, hipStream_t st);
void launch_runs_form(const unsigned *ikeys, const unsigned *ipos, long n, unsigned num_item, const unsigned *prev, int R, unsigned *head, unsigned *head_of,
                      unsigned char *idx, hipStream_t st);
void launch_runs_fill(const unsigned *user, const unsigned *item, const float *label, long n, const unsigned *unit_at, const unsigned *head_of,
                      const unsigned char *idx, long nunit, unsigned *c_item, unsigned *c_user, float *c_label, hipStream_t st);
// user-run units of rank pairs (svdf_k_wave.hip: k_pair_units); out != nullptr: scores only
bool pair_units_applies(const DevParams &P);
void launch_pair_units(const DevParams &P, const PairUnitSchedule &S, long begin, long end, float *out, hipStream_t st);
void launch_runs_iota(unsigned *v, long n, hipStream_t st);
void launch_runs_fill_u32(unsigned *v, long n, unsigned x, hipStream_t st);
// operand staging of a runs data set (knob "runs_stage"): dst[] / first[] from the level-sorted columns S and the schedule's order (ka .. vb: (1 + R) * nunit
// words each, pos_of: nunit; first: nrow = num_user + num_item words; row0 = the W row of user 0), and the copy of every touched row into its first slot
// (ns = 1 + R: slot s * ns + j, its row at row j * nunit + s of stage_row)
void launch_runs_stage_links(const RunSchedule &S, const int *order, long nunit, int R, unsigned num_user, unsigned row0, unsigned *pos_of, unsigned *ka, unsigned *kb,
                             unsigned *va, unsigned *vb, void **tmp, size_t *tmp_bytes, unsigned *dst, unsigned *first, long nrow, hipStream_t st);
void launch_runs_stage_in(const DevParams &P, const unsigned *first, long nrow, unsigned row0, float *stage_row, float *stage_bias, int ns, long nunit, hipStream_t st);
// ... and the labels next to the run-major slots: out[s * R + j] = S.label[j][s]
void launch_runs_label_rm(const RunSchedule &S, long nunit, int R, float *out, hipStream_t st);
// in-level order of the runs (knob "runs_order"): key[un] = (R - length) * num_item + item over the columns in unit-number order; over the level-sorted
// columns S: tot[0] = sum over the aligned sets of `ips` runs (from each level's begin) of the set's longest run, tot[1] = sets whose runs differ in length,
// tot[1 + length] = runs of that length
void launch_runs_order_key(const unsigned *c_item, const unsigned *c_user, long nunit, int R, unsigned num_item, unsigned *key, hipStream_t st);
void launch_runs_order_deal(const int *order, int *out, const long *level_ptr, int nlev, long nunit, int ips, hipStream_t st);
void launch_runs_order_stats(const RunSchedule &S, const long *level_ptr, int nlev, long nunit, int R, int ips, unsigned long long *tot, hipStream_t st);
bool basicmf_runs_soa_applies(const DevParams &P);
void launch_basicmf_runs_soa(const DevParams &P, const RunSchedule &S, long begin, long end, int R, int G, int block_threads, hipStream_t st);
void device_sort_pairs_u32(unsigned *keys_in, unsigned *keys_out, unsigned *vals_in, unsigned *vals_out, long n, void **tmp, size_t *tmp_bytes, hipStream_t st);
int sqerr_partials_grid(long n);
void launch_sqerr_partials(const float *pred, const float *label, long n, float scale, double *partials, hipStream_t st);
// ---- rank-pair sampling on the device (svdf_k_sample.hip)
struct RankSourceDev {          // a user-group buffer file resident in HBM, rows of shape (0 globals, 1 user entry, 1 item entry)
    long num_block, num_row;
    const long *block_row_ptr;  // [num_block + 1]
    const float *label, *uval, *ival;
    const unsigned *uidx, *iidx;
};
struct SamplerParams { float pos_lowerb, neg_upperb; int sample_num, sample_max; };
struct PairColumns { float *label, *uval, *v0, *v1; unsigned *uidx, *i0, *i1; };   // generated instances, file order
// the general device sampler (any row shape, both sampling methods, pointwise output): svdf_k_gsample.hip
struct RankRowsDev {            // a user-group buffer file's rows resident in HBM, reference CSR layout
    long num_block, num_row;
    const long *block_row_ptr;  // [num_block + 1]
    const float *label;         // [num_row]
    const int *row_ptr;         // [3 * num_row + 1]
    const unsigned *index;
    const float *value;
};
struct GSamplerParams { float pos_lowerb, neg_upperb, gap; int sample_num, sample_max, method, method_raw, pointwise; };
void launch_gsample_counts(const RankRowsDev &S, const GSamplerParams &sp, int *scratch, long *draws, long *pairs, hipStream_t st);
void launch_gsample_pairs(const RankRowsDev &S, const GSamplerParams &sp, const long *draw_off, const long *pair_off, const unsigned *raw, int *pos_list,
                          int *neg_list, int *pair_p, int *pair_n, hipStream_t st);
void launch_gpair_sizes(const RankRowsDev &S, const GSamplerParams &sp, long npairs, const int *pair_p, const int *pair_n, int *lens, hipStream_t st);
void launch_gpair_write(const RankRowsDev &S, const GSamplerParams &sp, long npairs, const int *pair_p, const int *pair_n, const int *optr, float *olabel,
                        unsigned *oi, float *ov, hipStream_t st);
void device_exclusive_scan_i32(const int *in, int *out, long n, void **tmp, size_t *tmp_bytes, hipStream_t st);
void host_sort_by_label(const float *label, long n, int *ids);
// std::sort of candidate ids by descending score as the reference's ranker does it (apex_svd_base.h:767), its partitions on nthreads threads
void host_parallel_sort_scores(const float *score, int *ids, long n, int nthreads);   // the restated std::sort (svdf_stdsort.h) on the host, for tests
void launch_rand_expand(const unsigned *tables, long nchunks, long C, long D, unsigned *raw, hipStream_t st);
// ---- window data sets of plain ratings / rank pairs (kind 5) regrouped on the device (svdf_k_wbuild.hip): the arrays of Engine::window_build.
// All pointers are device pointers; E = n (ratings) or 2 n (pairs) item entries.
struct WBuildIn { long n; int pairs; const unsigned *user, *item, *neg; const float *label; long num_user, num_item; };
struct WBuildBuffers {
    unsigned *k0, *k1, *v0, *v1;   // [E] sort ping-pong
    unsigned *inst;                // [n] instances in (user, file order)
    int *slot_e;                   // [E] slot of every item entry
    int *head, *mark;              // [n]
    int *run_user, *run_start, *run_begin;   // [n]
    void *tmp; size_t tmp_bytes;   // wbuild_tmp_bytes(E)
    unsigned *state;               // [8]
};
struct WBuildOut { WinUser *urec; unsigned *item, *item1; float *label, *v0, *v1; int *slot, *slot1, *iptr;
                   int *pos; };   // pos: nullptr, or [n] the source position of every regrouped instance (resident data sets: scoring in file order)
size_t wbuild_tmp_bytes(long m);
void device_window_build(const WBuildIn &in, const WBuildBuffers &B, const WBuildOut &out, long *nact, long *item_lo, long *item_hi, hipStream_t st);
// ---- the window rule of a sequence of rank-pair windows on a pass the device sampler left in HBM (svdf_k_rankwin.hip).
// columns: the sampler's merged item entries (i0, v0, i1) of unit-value rows -> pos / neg item per pair, count[item] += entries (integer atomics),
// keys / vals (nullptr: not wanted) = the 2 n entries' item and index for the sort; state[0] collects RW_ERR_* bits (such pairs are counted nowhere)
enum { RW_ERR_USER = 1, RW_ERR_ITEM = 2, RW_ERR_SAME = 4 };
void launch_rank_window_columns(long n, const unsigned *user, const unsigned *i0, const float *v0, const unsigned *i1, long num_user, long num_item,
                                unsigned *pos, unsigned *neg, unsigned *keys, unsigned *vals, unsigned *count, unsigned *state, hipStream_t st);
// the same kernel on columns that are pos / neg already (a pair source's draw, section 6ac): checks, counts and keys, nothing to turn back
void launch_rank_window_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg, long num_user, long num_item, unsigned *keys, unsigned *vals,
                              unsigned *count, unsigned *state, hipStream_t st);
size_t rank_window_sort_bytes(long E);
void rank_window_sort(void *tmp, size_t tmp_bytes, const unsigned *keys, unsigned *keys_sorted, const unsigned *vals, unsigned *vals_sorted, long E, long num_item,
                      hipStream_t st);
// for W windows cut at n w / W: the sum over (item, window) of c^2 and the largest c, c = the item's entries in the window.  Synchronizes st.
void rank_window_sums(const unsigned *keys_sorted, const unsigned *vals_sorted, long E, long n, long W, unsigned long long *d_out, unsigned long long *sum,
                      unsigned long long *worst, hipStream_t st);
// ---- SVDModel::rand_init on the device (svdf_k_init.hip): the j-th matrix element is the j-th accepted attempt of the polar loop
struct InitSeg { long begin, count; long row0; int k; float sigma; int absf; };   // elements [begin, begin + count) -> rows row0.. of W, k per row
struct InitPlan { InitSeg seg[3]; int nseg; long total; int pitch; double margin; };
struct InitReport { long j; unsigned r1, r2; };   // an element whose double lies within `margin` of a float rounding boundary, with its two raw draws
void launch_init_expand(const unsigned *tables, long nchunks, long C, long D, unsigned *raw, hipStream_t st);
size_t init_scan_tmp_bytes(long A);
void launch_init_patch(long n, const long *idx, const float *val, float *W, hipStream_t st);
void launch_init_tile(const unsigned *raw, long A, long base, const InitPlan &plan, float *W, unsigned *flag, unsigned *off, void *tmp, size_t tmp_bytes,
                      unsigned long long *state, InitReport *reports, int report_cap, hipStream_t st);
void launch_sample_counts(const RankSourceDev &S, const SamplerParams &sp, long *draws, long *pairs, hipStream_t st);
void launch_sample_posneg(const RankSourceDev &S, const SamplerParams &sp, const long *draw_off, const long *pair_off, const unsigned *raw,
                          int *pos_list, int *neg_list, const PairColumns &out, hipStream_t st);
// device-resident columns (already in HBM, file order) -> level schedule + level-sorted copies; see Engine::schedule_device_columns
// ---- conflict-free level scheduling on the device (svdf_k_sched.hip).  Unit u touches the parameter rows off[s] + col[s][u]
// for its K slots (SLOT_ABSENT = none; ids >= limit[s] raise limit_msg[s]); no row may repeat inside a unit.  Writes the
// level-sorted unit order (ties: sort_key, then file position -- the order of the host scheduler's stable sorts) to the
// device array order_out[n] and the level boundaries to level_ptr; returns the number of levels.  Throws std::runtime_error.
#define SVDF_SCHED_MAX_SLOTS 8
struct SchedColumns {
    int K;
    long n;
    const unsigned *col[SVDF_SCHED_MAX_SLOTS];     // device pointers, file order
    unsigned off[SVDF_SCHED_MAX_SLOTS], limit[SVDF_SCHED_MAX_SLOTS];
    const char *limit_msg[SVDF_SCHED_MAX_SLOTS];
    unsigned num_res;                               // resource ids are < num_res
    const unsigned *sort_key;                       // device, per unit; nullptr = file order inside a level
    unsigned sort_key_max;
};
long device_schedule(const SchedColumns &in, int *order_out, std::vector<long> &level_ptr, long *max_level_size, hipStream_t st);
// ---- the same for USER UNITS (SVD++ blocks; Engine::schedule_units, svdf_sched.cpp): unit u touches the rows of its instances
// [row_begin, row_end) of the staged CSR (global ids at goff, user ids at user_off, item ids at item_off), its feedback list at fb_off and,
// with UNIT_LOAD / UNIT_SAVE, the state resource.  Also decides the host scan's by-products: which units take the one-wave-per-user kernel
// (simple_out, 0 / 1 per unit), which rows repeat an item inside such a unit (fresh_out, per row), whether every simple unit has unit values.
struct UnitSchedIn {
    long n, nrow;
    const DevUnit *units;          // device, file order (flags without UNIT_SIMPLE)
    const int *row_ptr;            // device, 3 * nrow + 1
    const unsigned *index;
    const float *value;
    const unsigned *fb_index;
    unsigned goff, user_off, item_off, fb_off, num_item, num_fb, state_res;   // resource ids; state_res = the last one
    int simple_ok, fast_ok;
};
struct UnitSchedOut {
    std::vector<long> level_ptr;
    long max_level_size;
    bool any_fresh, unit_values;
};
long device_schedule_units(const UnitSchedIn &in, int *order_out, unsigned char *simple_out, unsigned char *fresh_out, UnitSchedOut &out, hipStream_t st);
void device_gather_u32(const unsigned *src, const int *order, unsigned *dst, long n, hipStream_t st);
void device_gather_f32(const float *src, const int *order, float *dst, long n, hipStream_t st);
void device_scatter_f32(const float *src, const int *order, float *dst, long n, hipStream_t st);   // dst[order[s]] = src[s]
// test probe: out[j] = device expf of in[j], or (in == nullptr) of the float with bit pattern first + j*step
int device_expf(const float *in, unsigned first, unsigned step, float *out, long n);

// ---- batch ranking evaluation on the live model (svdf_k_rankeval.hip): one piece of whole sections.  Every index is
// local to the piece and has been validated on the host.  A ROW of the sweep is a section or, for a section with more positives than a
// tile keeps thresholds, a slice of its positives; consecutive rows hold consecutive positives.
constexpr int RANK_EVAL_TILE_POS = 512;   // thresholds (positives) one sweep tile keeps in LDS; also the most positives of one row
struct RankEvalDev {
    int nsec;                   // sections of the piece
    const unsigned *sec_user;   // [nsec]
    const float *user_rows;     // nullptr: section s scores with the W_user row of sec_user[s]; else with row s of this [nsec][pitch] workspace (RankLiveRowsDev)
    const float *item_rows = nullptr, *item_bias = nullptr;   // nullptr: W_item / i_bias where the model keeps them; else the prepared [num_item][pitch] matrix and [num_item] biases (launch_rank_live_items)
    const int *sec_p0;          // [nsec + 1] positives of section s: [sec_p0[s], sec_p0[s + 1])
    long npos;
    const int *pos_item, *pos_sec;   // [npos]
    float *pos_score;                // [npos] written by k_rank_eval_pos
    int *greater, *tied, *before;    // [npos] zeroed by the caller
    int *nan_cnt;                    // [nsec] ranked candidates with a NaN score, zeroed by the caller
    int nrow, ntile;
    const int *row_sec, *row_first;  // [nrow] the row's section; 1 on the first row of a section (it counts the NaNs)
    const int *row_p0;               // [nrow + 1]
    const int *tile_r0;              // [ntile + 1] rows of tile t: at most rank_eval_tile_rows() of them, at most RANK_EVAL_TILE_POS positives
    long nban;
    const int *ban_sec, *ban_item;   // [nban] distinct (section, banned id) pairs
};
constexpr int RANK_EVAL_WIDE_ROWS = 32768;   // rows of one launch of the wide sweep (grid.y is at most 65535)
int rank_eval_tile_rows(const DevParams &P);
void rank_eval_geometry(const DevParams &P, long ntile, int *gy, long *items_per_block);   // item ranges of the narrow sweep over ntile row tiles; wide: one
void launch_rank_eval(const DevParams &P, const RankEvalDev &D, hipStream_t st);   // positives' scores, the counting sweep, the ban correction

// ---- top-N item lists on the live model (svdf_k_ranktopn.hip): one piece of whole sections.  The sweep keeps, per
// (section, item range y), a list of up to `cap` 64-bit keys (order-preserving score word << 32 | ~item id) in `list`; the merge selects the
// top_n largest keys of a section's gy lists.  Every index is local to the piece and has been validated on the host.
constexpr int RANK_TOPN_MAX = 256;       // largest top_n
constexpr int RANK_TOPN_MAX_CAP = 512;   // keys one wave sorts in LDS: the largest list capacity
struct RankTopnDev {
    int nsec;                        // sections of the piece
    const unsigned *sec_user;        // [nsec]
    const float *user_rows;          // nullptr: W_user rows; else the [nsec][pitch] workspace of effective user rows (RankLiveRowsDev)
    const float *item_rows = nullptr, *item_bias = nullptr;   // nullptr: W_item / i_bias; else the prepared item matrix and biases (launch_rank_live_items)
    const int *ban_p0;               // [nsec + 1] banned ids of section s: ban_item[ban_p0[s] .. ban_p0[s + 1]), distinct, ascending
    const int *ban_item;
    int top_n, cap, gy;              // list capacity (rank_topn_cap), item ranges (rank_topn_geometry)
    long items_per_block;            // items of one range
    unsigned long long *list;        // [nsec][gy][cap]
    int *list_cnt;                   // [nsec][gy] keys in the list, written by the sweep
    int *nan_cnt;                    // [nsec] ranked candidates with a NaN score, zeroed by the caller
    int *item_out;                   // [nsec][top_n] ids in rank order, -1 beyond count_out
    float *score_out;                // [nsec][top_n] their scores, 0 beyond count_out
    int *count_out;                  // [nsec] entries listed; 0 for a section with a NaN among its ranked candidates
};
int rank_topn_cap(const DevParams &P, int top_n);   // capacity of one list, <= RANK_TOPN_MAX_CAP
int rank_topn_tile_rows(const DevParams &P);        // sections that share one pass over an item range: 64 (narrow) or 1 (wide)
void rank_topn_geometry(const DevParams &P, long nsec, long max_lists, int *gy, long *items_per_block);   // at most max_lists / nsec (>= 1) item ranges
void launch_rank_topn(const DevParams &P, const RankTopnDev &D, hipStream_t st);   // the selecting sweep, then the merge: two launches

// ---- the effective user rows of a piece's sections on a user-group trainer (svdf_k_rankrows.hip):
// rows[s] = (0 + sum_j W_ufeedback[fb_index[j]] * fb_value[j], j in [fb_p0[s], fb_p0[s + 1]) in list order) + W_user[sec_user[s]] * 1, in the
// ranker's unfused fp32 arithmetic.  Every index is local to the piece and has been validated on the host.
struct RankLiveRowsDev {
    int nsec;
    const unsigned *sec_user;   // [nsec]
    const int *fb_p0;           // [nsec + 1]
    const unsigned *fb_index;   // feedback ids, < num_ufeedback
    const float *fb_value;
    float *rows;                // [nsec][pitch]
    // section 6z, ul_p0 != nullptr: the section brings a USER line instead of sec_user -- behind the feedback sum (fb_p0 == nullptr: 0), per entry
    // j in [ul_p0[s], ul_p0[s + 1]) in line order: += W_user[ul_index[j]] * ul_value[j], then the children of that id in P.feat_user
    const int *ul_p0 = nullptr;           // [nsec + 1]
    const unsigned *ul_index = nullptr;   // user ids, < num_user
    const float *ul_value = nullptr;
};
void launch_rank_live_rows(const DevParams &P, const RankLiveRowsDev &D, hipStream_t st);   // one launch
// the prepared item side of a trainer with a feature_item table: item_rows[i] = W_item[i] * 1 + its children's rows * cval, item_bias[i] alike
void launch_rank_live_items(const DevParams &P, float *item_rows, float *item_bias, hipStream_t st);   // one launch

// ---- the item side of svdf_item_topn (svdf_k_itemrows.hip)
// unit[i] = W_item[i] / sqrt(<W_item[i], W_item[i]>) element by element, +0 where the sum of squares is 0; [num_item][pitch], pads 0
void launch_item_unit_rows(const DevParams &P, float *unit, hipStream_t st);   // one launch
// rows[s] = base[item[s]] for the nsec sections of a piece; base is a [num_item][pitch] matrix (W_item or the unit rows), item[s] < num_item
void launch_item_query_rows(const DevParams &P, const float *base, const unsigned *item, int nsec, float *rows, hipStream_t st);   // one launch

// ---- ranking over per-section candidate lists on the live model (svdf_k_rankcand.hip): one piece of whole sections.
// Pair q of the piece is (section, cand_id[q]); a section's pairs are consecutive, its ids distinct and ascending.  Only the listed pairs
// are scored.  Every index is local to the piece and has been validated on the host.
struct RankCandDev {
    int nsec;                        // sections of the piece
    const unsigned *sec_user;        // [nsec]
    const float *user_rows;          // nullptr: W_user rows; else the [nsec][pitch] workspace of effective user rows (RankLiveRowsDev)
    const float *item_rows = nullptr, *item_bias = nullptr;   // nullptr: W_item / i_bias; else the prepared item matrix and biases (launch_rank_live_items)
    const int *sec_q0;               // [nsec + 1] pairs of section s: [sec_q0[s], sec_q0[s + 1])
    const int *cand_id;              // [npair]
    float *cand_score;               // [npair] written by the score kernel
    int ntile;
    const int *tile_q0, *tile_sec;   // [ntile + 1], [ntile]: at most 64 consecutive pairs of ONE section (svdf_rankcand_lists.h)
    // positions (top_n == 0): positive p of section s, p in [sec_p0[s], sec_p0[s + 1]), is pair pos_at[p]
    long npos = 0;
    const int *sec_p0 = nullptr, *pos_at = nullptr;
    int *position_out = nullptr, *tied_out = nullptr;   // [npos] strictly higher + tied with a smaller id; tied
    int *nan_out;                    // [nsec] 1: a pair of the section scored NaN
    // top-N (top_n >= 1): section 6x's layout
    int top_n = 0;
    int *item_out = nullptr;         // [nsec][top_n] ids in rank order, -1 beyond count_out
    float *score_out = nullptr;      // [nsec][top_n] their scores, 0 beyond count_out
    int *count_out = nullptr;        // [nsec] entries listed; 0 for a section with a NaN among its pairs
};
// form: 0 the measured choice per row width, 1 one lane per pair, 2 a wave per tile staging the gathered rows in LDS (pitch <= 256 only)
int rank_cand_form(const DevParams &P, int form);   // the form a piece's score kernel takes: 1 or 2
void launch_rank_cand(const DevParams &P, const RankCandDev &D, int form, hipStream_t st);   // the scores, then the count or the selection: two launches

// ---- the negatives of sampled-negative ranking, drawn on the device (svdf_k_ranknegs.hip): one piece of whole
// sections.  A section with positives has npos + num_neg pairs in cand_id, [sec_q0[s], sec_q0[s + 1]): its positives, then its negatives in
// draw order; a section without positives has none.  Every index is local to the piece and has been validated on the host.
struct RankNegsDev {
    int nsec;                  // sections of the piece
    long sec0;                 // the index IN THE CALL of the piece's first section: the stream of section s is that of sec0 + s
    uint64_t seed;
    unsigned num_item;
    int num_neg;               // 1 .. RANK_NEGS_MAX
    int slots, shift;          // the table of seen ids in LDS: rank_negs_table(num_neg) slots, shift = 32 - log2(slots)
    const int *sec_q0;         // [nsec + 1]
    const int *sec_p0;         // [nsec + 1] positives of section s: pos_id[sec_p0[s] .. sec_p0[s + 1])
    const int *pos_id;
    const int *ex_p0;          // [nsec + 1] excluded ids of section s (bans and positives): ex_id[ex_p0[s] .. ex_p0[s + 1]), distinct, ascending
    const int *ex_id;
    int *cand_id;              // [npair] written here, read by launch_rank_cand
    int *neg_out;              // nullptr, or [nsec][num_neg]: the negatives in draw order, -1 for a section without positives
};
void launch_rank_negs(const RankNegsDev &D, hipStream_t st);   // one launch, a wave per section

// ---- the negatives of a pass of rank pairs drawn from a pair source (svdf_k_pairdraw.hip): pair q = r * num_neg + j
// of source row r.  Every id has been validated on the host when the source was created.
struct PairDrawDev {
    long npair;                // n * num_neg, below 2^31 - 16
    int num_neg;               // 1 .. PAIR_SRC_MAX_NEG
    uint64_t seed;
    unsigned num_item;
    const unsigned *user;      // [n] the source's rows
    const unsigned *pos;       // [n]
    const int *uptr;           // [num_user + 1] the distinct items of user u: uitems[uptr[u] .. uptr[u + 1]), ascending
    const unsigned *uitems;
    unsigned *out_user;        // [npair] the pass's columns; out_user and out_pos may both be nullptr (svdf_pair_source_draw)
    unsigned *out_pos;
    unsigned *out_neg;
    unsigned *flag;            // one word, zeroed by the caller: q + 1 of a pair (any of them) that exhausted its draws
};
// T: the weight table of a weighted source (section 6ae; svdf_pairweight_lists.h), T.cdf == nullptr without one; wform: knob pair_weight_form
int pair_weight_form(long num_item, int form);   // the form a weighted draw takes: 1 (search of the whole cdf) or 2 (guided search)
void launch_pair_draw(const PairDrawDev &D, const PairWeightDev &T, int wform, hipStream_t st);   // one launch, a lane per pair
void launch_pair_weight_lookup(const PairWeightDev &T, int wform, long nx, const uint64_t *x, unsigned *id_out, hipStream_t st);   // the probe svdf_pair_weight_lookup

// ---- the hard pass of a pair source (svdf_k_pairhard.hip): pair q takes the best-scoring of its num_cand candidates,
// candidate i of pair q being the plain rule's negative of pair index q * num_cand + i.  D.npair counts the PAIRS of the pass (n * num_neg);
// npair * num_cand stays below 2^31 - 16.  The flag names an exhausted ENTRY: q * num_cand + i + 1.
struct PairHardDev {
    PairDrawDev D;
    int num_cand;              // 1 .. PAIR_HARD_MAX_CAND
    float *out_score;          // [npair] the chosen candidate's score, or nullptr
};
int pair_hard_form(const DevParams &P, int form, int num_cand);   // the form a hard pass's kernel takes: 1 (a lane per entry, rows where they lie) or 2 (staged)
void launch_pair_hard(const DevParams &P, const PairHardDev &H, const PairWeightDev &T, int wform, int form, hipStream_t st);   // one launch, a wave owns whole pairs

// ---- the rows of a shuffled pass of a pair source (svdf_k_pairorder.hip): position p holds source row sigma(p)
// (svdf_pairorder_lists.h).  The two columns written here are the `user` and `pos` of the PairDrawDev of the pass.
struct PairOrderDev {
    long n;                    // rows of the source, below 2^31 - 16
    PairOrderKeys K;           // pair_order_keys(order_seed, n)
    const unsigned *user;      // [n] the source's rows
    const unsigned *pos;       // [n]
    unsigned *out_user;        // [n] user[sigma(p)]
    unsigned *out_pos;         // [n] pos[sigma(p)]
    unsigned *flag;            // one word, zeroed by the caller: p + 1 of a position (any of them) that exhausted its walk
    unsigned *same;            // one word, zeroed by the caller: positions p >= 1 whose user is that of position p - 1
};
void launch_pair_order(const PairOrderDev &D, hipStream_t st);   // one launch, a lane per position

}  // namespace svdf
#endif

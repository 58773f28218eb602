/*
 * svdfeature_amd.h -- C ABI of the MI355X-native apex_svd SGD engine (libsvdfeature_amd.so).
 *
 * This is the drop-in boundary for ONE path of Gnnng/SVDFeature: the SGD training/prediction step
 * behind `class apex_svd::ISVDTrainer` (reference apex_svd.h:33-107), as implemented by the
 * reference's base solver (solvers/base-solver/apex_svd_base.h: SVDFeature :79-479, SVDPPFeature
 * :484-592).  The reference has no FFI layer of its own -- solvers are swapped at link time by
 * providing `apex_svd::create_svd_trainer` (apex_svd.h:212, solvers/base-solver/Makefile:17-23) --
 * so every entry point below is one ISVDTrainer virtual flattened to C: plain pointers and
 * sizes, no C++ or torch types.  `integration/apex_svd_amd.cpp` is the C++ class deriving
 * from the reference's own ISVDTrainer that forwards to these functions (INTEGRATION.md shows the
 * reference-side link line).
 *
 * Error behaviour follows the reference (apex-utils/apex_utils.h:47-58: message on stderr, then
 * exit(-1)) unless svdf_set_error_mode(1) was called, in which case a failing call returns a
 * negative status / NULL and svdf_last_error() holds the message.  Index-bound violations
 * ("user feature index exceed bound", apex_svd_base.h:320,327,343,360,530) are detected when
 * instances are staged, before anything reaches the GPU.
 *
 * Threading: like the reference a handle is driven from one thread at a time.
 * Borrowed pointers (instances, blocks) are copied before the call returns.
 */
#ifndef SVDFEATURE_AMD_H_
#define SVDFEATURE_AMD_H_

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svdf_trainer svdf_trainer; /* opaque: one ISVDTrainer instance */
typedef struct svdf_dataset svdf_dataset; /* opaque: a scheduled, HBM-resident training set */
typedef struct svdf_ranker svdf_ranker;   /* opaque: one ISVDRanker instance */
typedef struct svdf_pair_source svdf_pair_source; /* opaque: positives resident in HBM, the source of rank-pair passes */

/* ---- library ---- */
const char *svdf_version(void);
/* 0 (default): reference behaviour, errors print and exit(-1).  1: errors return status codes. */
void svdf_set_error_mode(int mode);
const char *svdf_last_error(void);
/* number of visible HIP devices (0 when there is no GPU; the library still loads). */
int svdf_device_count(void);

/* ---- lifecycle: apex_svd::create_svd_trainer(SVDTypeParam) (apex_svd.h:212; the four bytes are
 * SVDTypeParam, apex_svd_model.h:242-261) and the virtual destructor (apex_svd.h:106).
 * device < 0 selects the current HIP device. */
svdf_trainer *svdf_create(uint8_t format_type, uint8_t active_type, uint8_t extend_type, uint8_t variant_type,
                          int device);
void svdf_destroy(svdf_trainer *t);

/* ISVDTrainer::set_param (apex_svd.h:42; keys: apex_svd_base.h:126-136, apex_svd_model.h:350-368
 * and :456-476, ParameterSet prefixes up:/ip:/uip:/gp: apex_svd_base.h:48-67).  Unknown keys are
 * ignored, model-shape keys are ignored once the model is allocated.  Extension keys (ignored by the reference): amd:gpus, amd:exchange,
 * amd:step, amd:contrib, amd:window, amd:window_per_target(_max), amd:relax_* (see svdf_set_knob below) and amd:shared_user_from = B
 * (shared user rows in the one-GPU window step).
 * amd:step on ONE GPU (opt-in; not the reference's sequential result, contract |dRMSE| <= 1e-4): `minibatch` trains with the window step,
 * `auto` decides between it and the exact levels from the data's dependency depth, `levels` (and no key) is the exact step.  The key covers
 * resident data sets (svdf_dataset_from_* + svdf_train_dataset) AND the staged route (svdf_update_csr / _csr_batch / _block, what the
 * reference's CLI drives): a chunk -- the rows staged between two flush points: stage_window rows, finish_round, predict,
 * save_model, set_round, set_param, destroy -- trains exactly as svdf_dataset_from_X(chunk) + svdf_train_dataset + svdf_dataset_destroy would
 * on the same handle state, X = triples (plain ratings), pairs (rank pairs in the generator's shape), csr (anything else on a random-order
 * trainer; amd:shared_user_from, side tables, window_shared_sub and window_item_sub as on the resident path) or blocks (user-group trainers: the automatic
 * flush waits for the open user's END -- for at most 4 x stage_window staged rows, then it flushes like the default route; at any flush with
 * a user still open, that user and its continuation keep the exact unit path, which is normal and not counted).  A chunk whose rows or configuration the
 * window step does not cover keeps the exact flush -- never an error; the first one prints one stderr line naming the rule.  `auto` decides
 * on the first chunk of at least device_schedule_min rows and keeps the decision until the next svdf_set_param.
 * WIDTHS of the window step.  num_factor <= 1024: plain ratings and rank pairs -- svdf_dataset_from_triples / _from_pairs under
 * minibatch / auto, staged chunks of those two shapes, the stand-alone windows svdf_dataset_window_from_triples / _from_pairs with
 * svdf_window_delta_pack / _apply / _apply_local, svdf_stratum_step and the item-range pieces, amd:gpus handles on such rows, window_hot_sub --
 * and, on the one-GPU window sequence of amd:step = minibatch alone, everything that takes the user-unit kernels: svdf_dataset_from_csr (rows with
 * global features or several user / item entries, amd:shared_user_from, side tables) and svdf_dataset_from_blocks (SVD++ blocks, with shared user
 * ids too), the buffer-file routes that end in them, fp32 and bf16 slots as at the narrow widths; svdf_predict_dataset / svdf_eval_dataset on all of
 * these (beyond 256 factors a whole wave owns a row, two to four float4 per lane).
 * num_factor <= 256: the other routes of user units, one lane group per row -- svdf_dataset_window_from_csr / _from_blocks (the N-rank builders,
 * amd:gpus > 1), the staged route, amd:step = auto -- and the lanes of ordered sub-steps: window_shared_sub / window_item_sub / window_block_sub /
 * window_pair_sub > 0.  Beyond their width the resident calls refuse with a message that names the knob or the call; a staged chunk keeps the
 * exact flush (counter 31) and `auto` keeps the exact levels (decision 3). */
int svdf_set_param(svdf_trainer *t, const char *name, const char *val);
/* apex_random::seed (apex-tensor/apex_random.h:42-44) -> srand; process-global like the reference. */
void svdf_seed(unsigned seed);
/* ISVDTrainer::init_model (apex_svd.h:58; apex_svd_base.h:146-149): alloc + SVDModel::rand_init (apex_svd_model.h:665-705) over the
 * libc rand() stream -- the reference's draws and values bit for bit, libc's generator left where the reference's calls would have left
 * it.  On a device handle the matrices are sampled IN HBM (svdf_k_init.hip): 70 M normals in 4.5 ms instead of 1.9 s. */
int svdf_init_model(svdf_trainer *t);
/* ISVDTrainer::load_model / save_model (apex_svd.h:47,52): byte-compatible with
 * SVDModel::load_from_file / save_to_file (apex_svd_model.h:570-660).  The caller owns the FILE*
 * and reads/writes the leading 4-byte SVDTypeParam itself (svd_feature.cpp:165-190). */
int svdf_load_model(svdf_trainer *t, FILE *fi);
int svdf_save_model(svdf_trainer *t, FILE *fo);
/* EXTENSION for loops that own their files (integration/svdf_train_bulk.c): the model file written BESIDE the next pass.  _begin snapshots the model
 * in HBM (ordered behind everything enqueued so far) and returns; a writer thread streams the snapshot into `fo` (the same bytes svdf_save_model
 * would have written at that moment); training may go on.  _end joins the writer (the caller then closes the file).  One save in flight per
 * handle; amd:gpus handles, host-only handles and the bilinear solver write synchronously inside _begin.  The reference's protocol
 * (ISVDTrainer::save_model returns with the file complete, svd_feature.cpp:184-191) is svdf_save_model above. */
int svdf_save_model_begin(svdf_trainer *t, FILE *fo);
int svdf_save_model_end(svdf_trainer *t);
/* ISVDTrainer::init_trainer (apex_svd.h:64; apex_svd_base.h:151-173, 499-503) */
int svdf_init_trainer(svdf_trainer *t);
/* ISVDTrainer::set_round / finish_round (apex_svd.h:72,77).  finish_round flushes staged work. */
int svdf_set_round(svdf_trainer *t, int nround);
int svdf_finish_round(svdf_trainer *t);

/* ---- random-order input: ISVDTrainer::update(const SVDFeatureCSR::Elem&) / predict(const Elem&)
 * (apex_svd.h:83,89).  index/value hold the global, user and item sections back to back exactly
 * like Elem::set_space (apex_svd_data.h:71-78).  update stages the instance; the sequential
 * result is materialised at the next flush point (finish_round, predict, save_model, set_round,
 * destroy, or when the staging window fills). */
int svdf_update_csr(svdf_trainer *t, float label, int num_global, int num_ufactor, int num_ifactor,
                    const unsigned *index, const float *value);
float svdf_predict_csr(svdf_trainer *t, float label, int num_global, int num_ufactor, int num_ifactor,
                       const unsigned *index, const float *value);
/* bulk forms over one SVDFeatureCSR block (apex_svd_data.h:109-127 member layout): equivalent to
 * calling update/predict on rows 0..num_row-1 in order. */
int svdf_update_csr_batch(svdf_trainer *t, int num_row, const float *row_label, const int *row_ptr,
                          const unsigned *feat_index, const float *feat_value);
int svdf_predict_csr_batch(svdf_trainer *t, int num_row, const float *row_label, const int *row_ptr,
                           const unsigned *feat_index, const float *feat_value, float *out);

/* ---- user-grouped input: ISVDTrainer::update(const SVDPlusBlock&) /
 * predict(std::vector<float>&, const SVDPlusBlock&) (apex_svd.h:97,104); fields of SVDPlusBlock
 * (apex_svd_data.h:376-393) passed flat.  out must hold num_row floats. */
int svdf_update_block(svdf_trainer *t, int num_ufeedback, int extend_tag,
                      const unsigned *index_ufeedback, const float *value_ufeedback,
                      int num_row, const float *row_label, const int *row_ptr,
                      const unsigned *feat_index, const float *feat_value);
int svdf_predict_block(svdf_trainer *t, int num_ufeedback, int extend_tag,
                       const unsigned *index_ufeedback, const float *value_ufeedback,
                       int num_row, const float *row_label, const int *row_ptr,
                       const unsigned *feat_index, const float *feat_value, float *out);

/* ---- HBM-resident training sets (removes the per-instance virtual call).
 * A dataset is the instance stream of one pass of svd_feature.cpp:220-248's inner loop, scheduled
 * once and kept in HBM; svdf_train_dataset(t, ds) == update(x) for every x in file order.
 * svdf_dataset_from_triples is the three-column form of SVDBasicLoader (apex_svd_data.cpp:32-67):
 * no global feature, one user id and one item id with value 1. */
svdf_dataset *svdf_dataset_from_csr(svdf_trainer *t, long num_row, const float *row_label, const int64_t *row_ptr,
                                    const unsigned *feat_index, const float *feat_value);
svdf_dataset *svdf_dataset_from_triples(svdf_trainer *t, long n, const unsigned *user, const unsigned *item,
                                        const float *label);
/* rank pairs (user, positive item, negative item) in three columns: the instance PairwiseRankGenerator emits for two rows
 * with one unit item entry each (apex_svd_data.cpp:828-860 merge by index with the negative's sign flipped, :905-911
 * label 1): no global entry, user:1, {min(pos,neg): +-1, max(pos,neg): -+1}.  svdf_train_dataset == update(x) for
 * every such instance in order.  pos_item[r] != neg_item[r]. */
svdf_dataset *svdf_dataset_from_pairs(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item,
                                      const unsigned *neg_item);
/* user-group form: equivalent to update(SVDPlusBlock b) for b = 0..num_block-1 in order (the content of a
 * user-group buffer file, apex_svd_data.cpp:558-595).  Block b has extend_tag[b], feedback entries
 * fb_index/fb_value[fb_ptr[b] .. fb_ptr[b+1]) and rows block_row_ptr[b] .. block_row_ptr[b+1] of the CSR
 * arrays (row_ptr has 3*num_row+1 entries over all rows).  Every START must be closed by its END. */
svdf_dataset *svdf_dataset_from_blocks(svdf_trainer *t, long num_block, const int *extend_tag, const int64_t *fb_ptr,
                                       const unsigned *fb_index, const float *fb_value, const int64_t *block_row_ptr,
                                       const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                       const float *feat_value);
/* The same, straight from the reference's binary buffer files: user_group_format 0 = the CSR buffer written by
 * tools/make_feature_buffer (SVDFeatureCSRFactory::create_buffer, apex_svd_data.cpp:118-195; block layout
 * apex_svd_data.h:200-230), 1 = the user-group buffer written by tools/make_ugroup_buffer (SVDPlusBlock
 * save/load, apex_svd_data.h:419-450; apex_svd_data.cpp:558-595).  Replaces the loader thread + one virtual
 * update() per instance of svd_feature.cpp:220-248 for callers that train whole passes. */
svdf_dataset *svdf_dataset_from_buffer_file(svdf_trainer *t, const char *path, int user_group_format);
/* input_type = 2 of the reference (input_type::BINARY_BUFFER_RANK, apex_svd_data.h:516, apex_svd_data.cpp:1330-1332): the
 * user-group buffer file seen through PairwiseRankGenerator (apex_svd_data.cpp:812-1025).  Every block's rows are
 * replaced by rank pairs (positive entries merged with the sign-flipped negative's, label 1), drawn with libc rand()
 * in the generator's call order, so a process seeded like the reference's (srand(seed), then svdf_init_model) trains
 * on the same pairs.  One call = one pass of the iterator: the reference re-draws the pairs every round, so build a
 * new dataset per round.  Sampler keys are taken from svdf_set_param like the reference's iterator takes them from the
 * config: pos_sample_lowerb, neg_sample_upperb, rank_sample_num, rank_sample_max, rank_sample_method (0, 1),
 * rank_sample_gap, rank_sample_pointwise, seed_sampler_bytime.  Needs format_type = 1.
 * "amd:step" on a one-GPU handle: `minibatch` (and `auto` for the passes after the one that chose the window step for this file) gives a window
 * sequence (kind 8).  A file of plain rows -- no globals, one user and one item entry per row, every value exactly 1, no feedback ids -- drawn
 * with rank_sample_method 0 and no pointwise output is drawn AND cut into rank-pair windows (kind-5 children) in HBM: nothing of the pass but
 * the per-item counts and a few scalars crosses PCIe (counters 7 and 37).  Every other file, a prefetched pass, knob
 * device_window = 0 or window_pair_sub > 0 keep the route they had: user-unit windows (kind-7 children) built from the drawn blocks on the
 * host, or the exact pass where the window step does not take the configuration.  Same draws and the same rand() position on every route. */
svdf_dataset *svdf_dataset_from_rank_buffer_file(svdf_trainer *t, const char *path);
/* Draws the NEXT pass on a background host thread (the sampler is host work on the mapped file and libc rand(); the
 * device can train the current pass meanwhile).  The next svdf_dataset_from_rank_buffer_file / svdf_rank_sample_buffer_file
 * call for the same path takes the prefetched pass; the pairs are the ones that call would have drawn itself as long as
 * nothing else calls rand() in between (the reference's round loop does not, svd_feature.cpp:272-283).  0 on success. */
int svdf_rank_prefetch_buffer_file(svdf_trainer *t, const char *path);
/* The same pass written to out_path as a user-group buffer file instead of being uploaded (host only, works on a
 * handle created with device = -2).  Returns the number of generated rows, -1 on error. */
int64_t svdf_rank_sample_buffer_file(svdf_trainer *t, const char *in_path, const char *out_path);
void svdf_dataset_destroy(svdf_dataset *ds);                     /* also valid after svdf_destroy of its trainer */
int svdf_train_dataset(svdf_trainer *t, svdf_dataset *ds);       /* one pass, asynchronous on the trainer's stream */
/* out[num_row], in FILE order: the order of the rows as they were handed to svdf_dataset_from_* / svdf_dataset_window_from_*.  Read-only scoring
 * against the model as it stands at the call (pending staged rows are flushed first).  Window data sets score too -- the window sequences of
 * "amd:step" = minibatch / auto and the stand-alone windows of svdf_dataset_window_from_* (every window keeps its rows' source positions,
 * 4 bytes per row): each value is bit-identical to svdf_predict_csr_batch (user-group data sets: svdf_predict_block) for the same row on the same
 * model; a rank pair is one row -- user value 1, the two items in index order with the negative's sign flipped.  A stand-alone window that
 * svdf_train_dataset has walked but whose sums are not applied yet (svdf_window_delta_*) is scored against the model WITHOUT those sums.  Only
 * the data sets of an "amd:gpus" handle are refused: their rows are regrouped rank by rank and keep no file order. */
int svdf_predict_dataset(svdf_trainer *t, svdf_dataset *ds, float *out);
/* dataset facts: 0 num_row, 1 number of conflict-free batches, 2 largest batch, 3 kernel kind
 * (0 = basicMF fused kernel, 1 = general sparse kernel, 2 = few-row fused kernel, 3 = SVD++ user units),
 * 4 algorithmic bytes per pass, 5 number of user units, 6 units on the register-resident
 * fast path, 7 a digest of the host-resident schedule (level boundaries, fast-path split, unit order),
 * 8 a window sequence's (kind 8) kind of windows: 5 plain ratings / rank pairs, 7 user units; -1 for any other data set,
 * 9 operand staging of a runs data set (knob runs_stage): 0 not built yet, 1 built, 2 refused (size gate or no memory: rows stay in W),
 * 10 bytes of its staging buffers,
 * 11 runs data sets, runs_wave_steps: the sum, over the aligned row sets a wave of the pass kernel carries (8 runs at k = 64, 4 at k = 128, from each
 * level's begin), of the set's longest run = the steps the waves walk per pass; 12 runs_mixed_sets: the row sets whose runs differ in length;
 * 13 the order inside a level the data set was built with (knob runs_order); 11 - 13 are -1 for any other data set */
int64_t svdf_dataset_info(const svdf_dataset *ds, int what);

/* ---- multi-GPU support: item-side parameters are replicated, each rank trains its
 * user shard, and the item-side deltas of a window are summed across ranks by the caller's
 * collective (RCCL all-reduce on the returned device buffer).
 *   svdf_item_delta_begin   snapshot item-side parameters (W_item, i_bias [, g_bias])
 *   svdf_item_delta_buffer  delta = current - snapshot, returned as ONE contiguous fp32 device
 *                           buffer of *count floats (caller all-reduces it in place)
 *   svdf_item_delta_apply   current = snapshot + (all-reduced) delta */
int svdf_item_delta_begin(svdf_trainer *t);
void *svdf_item_delta_buffer(svdf_trainer *t, int64_t *count);
int svdf_item_delta_apply(svdf_trainer *t);
/* copy the packed delta to / from a caller-owned DEVICE buffer (e.g. a torch tensor the collective
 * runs on); both enqueue on the trainer's stream and return after it has drained. */
int svdf_item_delta_export(svdf_trainer *t, float *device_dst);
int svdf_item_delta_import(svdf_trainer *t, const float *device_src);
/* stream-ordered forms without host synchronisation: write (current - snapshot) straight into a caller-owned
 * device buffer / set current = snapshot + caller's buffer.  Both only enqueue on the trainer's stream; use
 * svdf_set_stream so the collective and these kernels share one stream order. */
int svdf_item_delta_into(svdf_trainer *t, float *device_dst, int64_t *count);
int svdf_item_delta_apply_from(svdf_trainer *t, const float *device_src);
/* the same in ONE launch over all replicated ranges and in the wire format of the collective: half = 0 packs fp32,
 * half = 1 packs IEEE fp16 (round to nearest even; parameters and arithmetic stay fp32).  device_dst = NULL only
 * returns *count (elements).  unpack sets current = snapshot + delta and, with refresh_snapshot != 0, also
 * snapshot = current, so the next window can pack again without svdf_item_delta_begin's copy. */
int svdf_item_delta_pack(svdf_trainer *t, void *device_dst, int half, int64_t *count);
/* The exchange of a window can be cut into nparts pieces by ITEM ID RANGE (part p = items [num_item*p/nparts, num_item*(p+1)/nparts);
 * ranges that are not indexed by item id travel with part 0): pack / unpack then cover the selected piece only, so the
 * all-reduce of one piece can run while the rank trains the instances whose items lie in another piece (no added staleness:
 * a piece's rows are not touched between its pack and its unpack).  svdf_item_delta_begin always snapshots everything. */
int svdf_item_delta_select(svdf_trainer *t, int part, int nparts);
int svdf_item_delta_unpack(svdf_trainer *t, const void *device_src, int half, int refresh_snapshot);

/* ---- window-minibatch step of the N-rank path (svdf_k_window.hip).  The reference has no counterpart: it
 * is single-process.  What is re-arranged is what ONE instance contributes in SVDFeature::update_no_decay +
 * regularize (solvers/base-solver/apex_svd_base.h:383-427, :286-311): the user-side change is applied at once (users are
 * private to a rank: exact sequential SGD), the item-side change is collected per window and applied after the all-reduce.
 *   ds = svdf_dataset_window_from_triples(t, ...)   one exchange window of this rank's shard (user % N == rank), grouped by user
 *   svdf_train_dataset(t, ds)                       every instance = the reference's update_inner on (current user side,
 *                                                   window-start item side); W_item / i_bias are NOT written
 *   svdf_window_delta_pack(t, ds, dst, half, &n)    dst = per item, the sum in file order of what its instances would have changed
 *                                                   (same packed layout / item-range partition as svdf_item_delta_pack; NULL dst = size)
 *   all-reduce(dst) over the ranks
 *   svdf_window_delta_apply(t, dst, half)           replicated ranges += dst
 * Deterministic (no float atomics); equals oracle/svdf_oracle.c: svdo_update_csr_batch_stale bit for bit with fp32 deltas. */
svdf_dataset *svdf_dataset_window_from_triples(svdf_trainer *t, long n, const unsigned *user, const unsigned *item, const float *label);
/* the same for rank pairs (user, positive item, negative item), the instances of svdf_dataset_from_pairs (BASELINE configs[4]) */
svdf_dataset *svdf_dataset_window_from_pairs(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item, const unsigned *neg_item);
/* The same step for USER UNITS (svdf_k_wunit.hip): rows with global features and / or several item entries
 * (random-order trainers: _from_csr, the arrays of svdf_dataset_from_csr) and user-group (SVD++) blocks (_from_blocks, the arrays of
 * svdf_dataset_from_blocks; every START closed by its END inside the window).  A user's unit is exact on its private state -- its W_user
 * row and bias and SVDPPFeature's tmp_ufeedback / old_ufeedback (solvers/base-solver/apex_svd_base.h:486-488, 506-520) --; the shared rows
 * -- W_item / i_bias, W_ufeedback / ufeedback_bias (prepare_ufeedback / update_ufeedback :523-554), g_bias (:188-210, :313-353) -- are
 * read as of the window start and their change is summed per row in file order: svdf_window_delta_pack writes the sums in the packed
 * layout [W_ufeedback | W_item | ufeedback_bias | i_bias | g_bias] (one piece: svdf_item_delta_select(t, 0, 1)),
 * svdf_window_delta_apply_local adds them to the model in place.  Every row needs exactly one user entry; ids are distinct inside a
 * row / a feedback list.  Equals oracle/svdf_oracle.c: svdo_update_csr_batch_stale / svdo_update_block_stale bit for bit. */
svdf_dataset *svdf_dataset_window_from_csr(svdf_trainer *t, long num_row, const float *row_label, const int64_t *row_ptr,
                                           const unsigned *feat_index, const float *feat_value);
svdf_dataset *svdf_dataset_window_from_blocks(svdf_trainer *t, long num_block, const int *extend_tag, const int64_t *fb_ptr,
                                              const unsigned *fb_index, const float *fb_value, const int64_t *block_row_ptr,
                                              const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                              const float *feat_value);
int svdf_window_delta_pack(svdf_trainer *t, svdf_dataset *ds, void *device_dst, int half, int64_t *count);
int svdf_window_delta_apply(svdf_trainer *t, const void *device_src, int half);
/* STRATIFIED schedule: item block b = the partition chosen with svdf_item_delta_select(t, b, N).  While a rank
 * trains a stratum (its users x one item block) it owns that block exclusively, so the window's per-item sums are added to the model in
 * place (no wire buffer, no sum over ranks); afterwards the block -- its W_item rows and i_bias words (global biases travel with block 0),
 * fp32, the packed layout of svdf_item_delta_pack -- is handed to the next rank: _get copies it out, _set copies a received block in.
 * device_dst = NULL only returns *count (floats). */
int svdf_window_delta_apply_local(svdf_trainer *t, svdf_dataset *ds);
int svdf_item_block_get(svdf_trainer *t, float *device_dst, int64_t *count);
int svdf_item_block_set(svdf_trainer *t, const float *device_src);
/* one stratum step in one call: every window data set trained (svdf_train_dataset) and summed in place into item block `block` of `nblocks`
 * (svdf_window_delta_apply_local), then -- device_out != NULL -- the block copied out for its hand-over; svdf_item_block_set_at puts an arrived
 * block in place.  The same launches as the calls they fuse (the host thread of a rank has ~40 us per step at 8 ranks). */
int svdf_stratum_step(svdf_trainer *t, svdf_dataset *const *windows, int num_windows, int block, int nblocks, float *device_out);
int svdf_item_block_set_at(svdf_trainer *t, int block, int nblocks, const float *device_src);
/* ---- cross-PROCESS direct exchange (svdf_ipc.cpp): one process per GPU, but the exchange of a window runs through
 * IPC-mapped device buffers -- every rank's wire buffer and flag page mapped into every process (over xGMI on distinct devices) -- with the
 * peer-pointer reduce-scatter + all-gather kernel of the amd:gpus handle, ordered across processes by sequence flags in device memory
 * (no collective library, no host rendezvous inside a pass).  The reference has no counterpart (single process).
 *   svdf_ipc_setup(t, rank, world, wire_bytes, block_floats, handles)   allocate + export; handles = 128 bytes to all-gather
 *   svdf_ipc_connect(t, all_handles)                                    world x 128 bytes in rank order
 *   per window: svdf_train_dataset(ds); svdf_ipc_window_pack(t, ds, half); svdf_ipc_window_reduce(t, half); svdf_ipc_window_apply(t, half)
 *   stratified hand-over: svdf_ipc_block_send(t, dst, slot) stores the active item block (svdf_item_delta_select) into rank dst's inbox;
 *   svdf_ipc_block_recv(t, src, slot, seq) waits for the seq-th block of rank src, puts it in place and acknowledges the slot.
 * A wait that hits its spin limit raises an error word instead of hanging the queue: svdf_ipc_status(t) != 0, later calls fail. */
int svdf_ipc_setup(svdf_trainer *t, int rank, int world, int64_t wire_bytes, int64_t block_floats, unsigned char *handles_out);
int svdf_ipc_connect(svdf_trainer *t, const unsigned char *all_handles);
int svdf_ipc_window_pack(svdf_trainer *t, svdf_dataset *ds, int half);
int svdf_ipc_window_reduce(svdf_trainer *t, int half);
int svdf_ipc_window_apply(svdf_trainer *t, int half);
int svdf_ipc_block_send(svdf_trainer *t, int dst_rank, int slot);
int svdf_ipc_block_recv(svdf_trainer *t, int src_rank, int slot, unsigned seq);
int svdf_ipc_status(svdf_trainer *t);
int svdf_ipc_close(svdf_trainer *t);

/* ---- the same exchanges issued from C++ straight into RCCL (svdf_rccl.cpp): one process per GPU, the rank's own communicator
 * (ncclCommInitRank on the trainer's device; librccl.so resolved at run time -- inside a torch process the library torch loaded), so that a
 * pass needs no Python call and no torch.distributed work object per collective.  Replaces, like the rest of section 6, the round loop of ONE
 * process (svd_feature.cpp:220-248) on N ranks.
 *   svdf_rccl_unique_id(out[128])                      rank 0; the bytes reach the other ranks through the caller's process group / store
 *   svdf_rccl_init(t, id, rank, world)
 *   all-reduce step, per window: svdf_train_dataset(ds); svdf_rccl_window_allreduce(t, ds, half)   (per-item sums -> ncclAllReduce in place -> add)
 *   stratified hand-over: svdf_rccl_block_handoff(t, dst, src, slot, in_block, nblocks) sends the ACTIVE item block (svdf_item_delta_select) to rank
 *   dst while block in_block of nblocks arrives from rank src into inbox slot `slot` (0 / 1), on a side stream ordered by events;
 *   svdf_rccl_block_arrive(t, slot) makes the trainer's stream wait for that transfer and puts the block in place (active partition = its block).
 *   svdf_rccl_counter: 0 hand-overs issued, 1 all-reduces issued. */
int svdf_rccl_unique_id(unsigned char *out128);
int svdf_rccl_init(svdf_trainer *t, const unsigned char *id128, int rank, int world);
int svdf_rccl_window_allreduce(svdf_trainer *t, svdf_dataset *ds, int half);
int svdf_rccl_block_handoff(svdf_trainer *t, int dst_rank, int src_rank, int slot, int in_block, int nblocks);
int svdf_rccl_block_arrive(svdf_trainer *t, int slot);
int64_t svdf_rccl_counter(svdf_trainer *t, int what);
int svdf_rccl_close(svdf_trainer *t);

/* test probe of the device rank sampler's sort (svdf_stdsort.h: libstdc++'s std::sort restated for host and device, because
 * PairwiseRankGenerator::sample_cmp, apex_svd_data.cpp:920-944, picks rows by POSITION after an unstable std::sort): ids 0..n-1
 * sorted by label with the restated code (restated[]) and with the C++ library's own std::sort (library[]). */
int svdf_debug_sort_labels(long n, const float *label, int *restated, int *library);
/* test probe of the ranker's tie-breaking sort (SVDFeatureRanker sorts its entry vector with std::sort, apex_svd_base.h:767; sections whose
 * scores tie are finished by exactly that sort, its partitions spread over `threads` host threads): ids 0..n-1 by descending score with
 * the threaded restatement (parallel[]) and with the library's std::sort over the reference's Entry struct (library[]). */
int svdf_debug_sort_scores(long n, const float *score, int threads, int *parallel, int *library);

/* ---- introspection used by tests, bench.py and the harness ---- */
/* raw copies of parameter views: 0 u_bias 1 W_user 2 i_bias 3 W_item 4 g_bias 5 ufeedback_bias
 * 6 W_ufeedback; rows are returned unpadded.  Returns number of floats or -1. */
int64_t svdf_get_view(svdf_trainer *t, int which, float *out, int64_t capacity);
int svdf_view_shape(svdf_trainer *t, int which, int *rows, int *cols);
/* overwrite a view from rows*cols unpadded floats (multi-GPU: every rank owns a slice of the user rows, the slices are
 * gathered before a model is saved).  Returns the number of floats or -1. */
int64_t svdf_set_view(svdf_trainer *t, int which, const float *in, int64_t count);
/* the HIP stream (hipStream_t) all of this trainer's work is enqueued on; timing code records
 * HIP events on it. */
void *svdf_stream(svdf_trainer *t);
/* adopt a caller-owned HIP stream (e.g. the stream a torch process group orders its collectives against);
 * pending work on the old stream is drained first.  The trainer never destroys an adopted stream. */
int svdf_set_stream(svdf_trainer *t, void *hip_stream);
int svdf_synchronize(svdf_trainer *t);
/* counters: 0 instances trained, 1 kernels launched, 2 conflict-free batches executed,
 * 3 staged-window flushes, 4/5/6 launches of the basicMF / general / few-row fused kernel, 7 rank passes sampled on the device,
 * 8..12 amd:gpus handles (exchanges, RCCL, distinct devices, window steps, exchange path), 13 / 14 the last svdf_init_model on the
 * device: values the host libm decided (next to a float rounding boundary) / rand() draws consumed (0 = the host loop ran), 15 conflict-free
 * levels executed inside chained launches, 16 .. 20 the decision of `amd:step = auto` for the data set built last (16: 0 none, 1 exact levels
 * kept, 2 window step chosen, 3 exact kept because the window step does not cover the configuration / the rows; 17 conflict-free levels;
 * 18 / 19 dag bound and stream model in microseconds; 20 windows), 21 unused,
 * 22 / 23 passes over hot-row units / runs, 24 microseconds the schedule of the last user-unit data set took, 25 whether the device built it,
 * 26 data sets whose DEFAULT (exact) step drew the depth warning (a stderr line naming `amd:step = auto`: the level schedule predicts the pass
 * more than 10 x slower than the streaming model), 27 / 28 the last noted data set's dag bound / stream model in microseconds,
 * 29 passes over rank pairs walked as user-run units,
 * 30 staged chunks trained by the window step (amd:step = minibatch / auto on the staged route of a one-GPU handle), 31 staged chunks kept
 * exact under those keys because their rows or the configuration are outside the window step, 32 depth warnings of the DEFAULT step about
 * staged chunks (the stderr line of 26 for svdf_update_*: at most one per handle; 26 .. 28 count resident data sets only),
 * 33 / 34 user-group (SVD++) windows with shared user entries (amd:shared_user_from) walked by the one-wave-per-unit form that
 * keeps a segment's shared rows in registers / by the general lane-group kernel,
 * 35 hot shared user rows applied in ordered sub-steps on such windows (knob window_block_sub; the windows count under 34),
 * 36 hot item rows applied in ordered sub-steps on user-group (SVD++) windows, with or without shared user entries (knob window_block_item_sub;
 * DESIGN.md 6u; the windows keep counting where they do without the knob),
 * 37 rank passes of a candidate file (svdf_dataset_from_rank_buffer_file) built as window sequences in HBM (they count under 7 too),
 * 38 sections ranked by svdf_rank_eval_positions, 39 sections listed by svdf_rank_topn,
 * 40 of the sections under 38 / 39, those ranked with a user row built from a feedback list (the _fb calls on user-group trainers),
 * 41 .. 43 see the _lines, _cand and _sampled calls below,
 * 44 / 45 passes built from a pair source (svdf_dataset_from_pair_source) without the pair columns leaving HBM / through
 * svdf_dataset_from_pairs' own builder on the columns copied back,
 * 46 of the passes under 44 / 45, the hard ones (svdf_dataset_from_pair_source_hard),
 * 47 of the passes under 44 / 45, those drawn from a source with item weights (svdf_pair_source_create_weighted),
 * 48 of the passes under 44 / 45, the shuffled ones (svdf_dataset_from_pair_source_shuffled),
 * 49 sections listed by svdf_item_topn */
int64_t svdf_counter(svdf_trainer *t, int what);
/* Tuning knobs (not part of the reference surface).  None changes a result bit except those marked (*), which move the windows of the
 * OPT-IN window step only.  Every knob, its default, what other values select (round 6: knobs no test or tool sets were deleted).
 *   staging / launches
 *     stage_window        2^21   instances staged by svdf_update_* before an automatic flush (also set by the config key amd:window)
 *     async_flush         1      full staged windows are scheduled on a background thread
 *     staged_pool         1      amd:step = minibatch / auto on the staged route: the per-chunk window sequence takes its device blocks from a
 *                                pool kept on the handle (0 = hipMalloc / hipFree per chunk: A/B, same bits)
 *     use_graph           0      1 = a resident data set's pass is replayed as a captured hipGraph
 *     groups_per_wave     0      lane-group sets per wave of the contract / few-row kernels (0 = tuned per width; 1..6, 8)
 *     block_threads       0      workgroup size (0 = tuned per width; 64, 128, 256)
 *     xcd_remap           1      blockIdx -> tile mapping that keeps neighbouring tiles on one XCD's L2 (0 = plain)
 *     load_mode           2      row gathers: 0 plain, 1 nontemporal, 2 = by row size
 *     store_mode          0      row stores: 0 plain, 1 nontemporal, 2 write-through
 *       These five shape the launch of ONE level by the level kernels; which forms each reaches (svdf_level_geometry reports it per launch):
 *         groups_per_wave  every k_basicmf / k_basicmf_slots form takes the value as it is (auto: 4 at 16 lanes per row, 2 at 64 lanes, 1 below and
 *                          for the sixteen-lane slots form; the eight-lane slots form min(4, max(1, (n + 7200) / 14400)) for a level of n).  k_fused
 *                          with at most three id slots folds every value >= 2 to 2 (auto: 2 at 16 lanes, else 1); k_fused with 2 + 2 slots, its
 *                          hot-reduce form and the few-row fast forms (k_fewrow_fast, k_fewrow_slots) ignore it: one row set per wave
 *         block_threads    every form but k_fused's hot-reduce form (1024 threads); auto: 64, but 256 for k_basicmf off 16 lanes per row
 *         xcd_remap        every form: the grid is padded to a multiple of 8 and the tiles permuted
 *         load_mode        k_basicmf, k_fused and k_fewrow_fast; the slots forms (k_basicmf_slots with eight and with sixteen lanes, k_fewrow_slots)
 *                          always gather nontemporal
 *         store_mode       the general instruction stream of k_basicmf only: a value other than 0 leaves the FAST and slots forms of the contract
 *                          configuration (and the chained and runs forms) for that stream; every other form stores plain and the few-row
 *                          launchers ignore the knob
 *       The chained launches (chain_width), the inline-global few-row form (fewrow_gslots), the runs pass and the hot-row units read none of them.
 *     sort_batches        1      order inside a conflict-free level: 0 file order, 1 by item, 2 by user
 *     chain_width         128    levels of at most this many instances are walked inside ONE launch by one workgroup (0 = a launch per level)
 *   kernel routing (0 = the more general kernel; same bits)
 *     use_fused 1, fewrow_i16 1, fewrow_gslots 1, basic_i8 1, use_simple_units 1, svdpp_helpers 8 (waves per SVD++ user: 1, 4, 8, 16),
 *     rows_without_feedback 1 (0 = whole users stay sequential units even when no block carries a feedback id)
 *   schedule forms of plain ratings
 *     runs_exec           1      runs of an item's consecutive ratings as units (svdf_k_runs.hip); runs_len 4 (2..7), runs_sets 1, runs_block 64,
 *                                runs_min_rows 2^20 (smaller data sets keep one instance per lane group)
 *     runs_stage          1      a run writes every row into its next reader's schedule slot instead of W (W is written at the row's last touch of a
 *                                pass and is the truth between passes; same bits).  Costs (1 + R) * runs * (4 k + 8) bytes of device memory, taken
 *                                only when that is at most half of the free memory and at most runs_stage_max_mb (-1 = no cap); 0 = rows live in W
 *     runs_store          1      cache policy of the staged runs kernel's stores (runs_stage 1 only; same bits): 0 = all plain; 1 = the 4-byte bias
 *                                words nontemporal, the rows plain; 2 = rows and bias words sc1 write-through.  Read at every pass
 *     runs_order          1      order of the runs inside a level, honoured with sort_batches 1: 1 = by length, longest first, then by item, the level's
 *                                row sets dealt round robin into the eight contiguous shares the XCDs take (a wave walks as many steps as its
 *                                longest run; same bits); 0 = by item.  Read when a data set is BUILT: changing it later does not touch an existing
 *                                data set (svdf_dataset_info 11 - 13).  Falls back to 0 when R * num_item does not fit 32 bits
 *     pivot_exec          1      hot rows walked as units (svdf_pivot.cpp); pivot_min 2048 (ratings that make a row hot), pivot_run 256 (per unit)
 *   schedule forms of rank pairs
 *     pair_units          1      user-grouped pair streams (the generator's own order: a user's pairs back to back) walked as user-run units
 *                                (svdf_punit.cpp: k_pair_units, the user's row in registers); pair_unit_cap 16 (pairs per unit at most)
 *   one-off builders on the device (0 = the host builder; same arrays / model)
 *     device_schedule 1 (device_schedule_min 2^16: smaller staged windows stay on the host), device_rank 1, device_init 1
 *     (device_init_margin_log2 46), device_window 1, device_load 1
 *   the opt-in window step (amd:step = minibatch / auto; N-rank handles)
 *     wunit_fast 2 (3: in addition the one-wave-per-unit form for user-group windows with shared user entries), wunit_inplace 1, wunit_defer_fb 1, window_slots 1, window_groups 0      kernel forms, same bits
 *     window_per_target (*) 24, window_per_target_fb (*) 16     updates a shared row / feedback row meets per window on average
 *     window_per_target_shared (*) 12                           ... a shared user row (amd:shared_user_from; profiles/r07_sidefeat_window.md)
 *     window_per_target_child (*) 3                             ... a feature_user / feature_item child row (profiles/r08_sidetable_window.md)
 *     window_per_target_max (*) 128                             ... and at most (N-rank steps, rank pairs, user units; plain ratings on one GPU with window_hot_sub = 0)
 *     window_count_actual (*) 1                                 one-GPU sequences of svdf_dataset_from_triples / _from_pairs / _from_csr (amd:step = minibatch / auto, the staged
 *                                                               chunks of svdf_update_* included): the means and the "at most" values of this table are counted on the
 *                                                               windows AS CUT (equal file positions), each times the slack 1.5, and the window count is raised until they hold --
 *                                                               a file sorted by item, one that arrives in bursts, one sorted by a shared user id gets many small windows instead
 *                                                               of NaN.  Enforced per window: mean over a class's entries of min(updates of the entry's row, sub-step of its lane)
 *                                                               <= 1.5 x its window_per_target*; no row of the class more than 1.5 x its cap (window_per_target_max, or the lane's
 *                                                               window_*_max).  The slack: a file in random order sits above the per-pass figures by the Poisson term (mean + 1; the
 *                                                               maximum by about 3 sigma), and must keep the windows of the calibrations (profiles/r17_window_orders.md).  amd:gpus > 1
 *                                                               enforces window_per_target_max alone, without slack.  NOT covered: user-group blocks (svdf_dataset_from_blocks):
 *                                                               window_per_target_fb, window_per_target_shared and window_block_max hold there ON AVERAGE over a pass's windows only.
 *                                                               amd:window overrides everything.  0 = the per-pass rule alone (A/B); part of the data set's schedule signature
 *     window_hot_sub (*) 128, window_hot_max (*) 2048           one-GPU sequences of plain ratings (round 6): an item with more than window_hot_sub slots in a window
 *                                                               moves in ordered sub-steps of that many (k_window_apply; 0 = off) and meets at most window_hot_max
 *                                                               updates per window -- the hottest item no longer sets the number of windows.  Set before the data set is
 *                                                               built: train_dataset refuses a sequence built with another window_hot_sub.  Every width (num_factor <= 1024)
 *     window_shared_sub (*) 0, window_shared_max (*) 512        one-GPU sequences of rows with shared user entries / feature_user children (amd:shared_user_from):
 *                                                               a shared user row (id >= B) with more than window_shared_sub slots in a window moves in ordered sub-steps
 *                                                               of that many (k_wunit_apply_shared; 0 = off, the default: the rule and bits of 6i / 6j) and meets at most
 *                                                               window_shared_max updates per window; the class means (window_per_target_shared / _child) then bound
 *                                                               min(updates per window, window_shared_sub).  Set before the data set is built: train_dataset refuses a
 *                                                               sequence built with another window_shared_sub.  Refused with amd:contrib = bf16, user-group trainers,
 *                                                               amd:gpus > 1 / svdf_dataset_window_from_csr.  12 with the defaults: 4.0x the 6i rule at |dRMSE| <= 6.9e-5
 *                                                               on the side-feature variant (profiles/r09_shared_hot.md); does not pay on the 6j table variant
 *     window_item_sub (*) 0, window_item_max (*) 2048           the same lane for the ITEM range of such sequences (any row set that takes the csr path: global features, shared user
 *                                                               ids, side tables): an item row -- a plain item entry's row, a feature_item child's row, or both --
 *                                                               with more than window_item_sub (0 .. 128) slots in a window moves in ordered sub-steps of that many
 *                                                               (k_wunit_apply_hot; 0 = off, the default: the rule and bits as before) and meets at most window_item_max
 *                                                               updates per window; the class means (window_per_target / _child) then bound min(updates per window,
 *                                                               window_item_sub).  Works with and without amd:shared_user_from and next to window_shared_sub.  Set before the
 *                                                               data set is built: train_dataset refuses a sequence built with another window_item_sub.  Refused with
 *                                                               amd:contrib = bf16, user-group trainers, amd:gpus > 1 / svdf_dataset_window_from_csr, wunit_inplace = 0.
 *                                                               Calibration: profiles/r11_item_hot.md
 *     window_block_sub (*) 0, window_block_max (*) 512          the same lane for the shared user rows of USER-GROUP (SVD++) blocks (amd:shared_user_from on a format_type 1 trainer,
 *                                                               svdf_dataset_from_blocks / svdf_dataset_from_buffer_file(.., 1) under amd:step = minibatch): a shared
 *                                                               user row with more than window_block_sub (0 .. 4096) slots in a window moves in ordered sub-steps of that many
 *                                                               (k_wunit_apply_hot, each slot from the span state its walk held: private row and bias, tmp_ufeedback and its
 *                                                               bias; 0 = off, the default: the rule and bits of 6p) and meets window_block_max updates per window on average (see window_count_actual);
 *                                                               window_per_target_shared then bounds the mean of min(updates per window, window_block_sub).  Without effect on
 *                                                               random-order trainers, without amd:shared_user_from and on blocks without shared ids.  Set before the data
 *                                                               set is built: train_dataset refuses a sequence built with another window_block_sub.  Refused with
 *                                                               amd:contrib = bf16, amd:gpus > 1 / svdf_dataset_window_from_blocks, wunit_inplace = 0 once a row is hot.
 *                                                               Measured on 64 dense buckets (profiles/r16_block_hot.md): 14x the 6p rule at the default cap, and the |dRMSE| <= 1e-4
 *                                                               contract missed with the knob on (3.5e-3) and off (1.3e-3): the cap is not a calibrated value
 *     window_block_item_sub (*) 0, window_block_item_max (*) 2048   OPT-IN.  The same lane for the ITEM rows of USER-GROUP (SVD++) blocks (format_type 1 trainers, with or without amd:shared_user_from;
 *                                                               svdf_dataset_from_blocks / svdf_dataset_from_buffer_file(.., 1) / staged svdf_update_block chunks under amd:step =
 *                                                               minibatch): an item row with more than window_block_item_sub (0 .. 128) slots in a window moves in
 *                                                               ordered sub-steps of that many (k_wunit_apply_hot<LPI, true, true>, each slot from the span state its walk held:
 *                                                               private row and bias, tmp_ufeedback and its bias; 0 = off, the default: today's rule and bits) and meets at most
 *                                                               window_block_item_max updates per window; window_per_target then bounds the mean of min(updates per window,
 *                                                               window_block_item_sub).  The range and meaning of window_item_sub, which stays refused with user-group trainers.
 *                                                               Without effect on random-order trainers and on windows in which no item is hot.  Set before the data set is
 *                                                               built: train_dataset refuses a sequence built with another window_block_item_sub.  Refused with amd:contrib =
 *                                                               bf16, amd:gpus > 1 / svdf_dataset_window_from_blocks, num_factor > 256, wunit_inplace = 0 once a row is hot.
 *                                                               Measured on Zipf(0.7) items (profiles/r22_block_item_hot.md): caps 512 .. 4 096 hold |dRMSE| <= 1e-4; 2 048 and 4 096 cut the
 *                                                               same windows there, so the default stays 2 048.  The lane is SLOWER than the knob at 0 on that input (0.86x at best:
 *                                                               windows with a hot row leave the one-wave-per-unit walk), and the feedback rows' term of the rule is not lowered by it
 *     window_pair_sub (*) 0, window_pair_max (*) 4096           the same lane for RANK PAIRS (svdf_dataset_from_pairs and pair-shaped staged chunks under amd:step = minibatch /
 *                                                               auto): an item with more than window_pair_sub (0 .. 128) slots in a window -- both signs counted --
 *                                                               moves in ordered sub-steps of that many (k_window_apply_pairs; 0 = off, the default: the rule and bits as
 *                                                               before), each slot evaluated against the pair's OTHER item as of the window start, and meets at most
 *                                                               window_pair_max updates per window; window_per_target then bounds the mean of min(updates per window,
 *                                                               window_pair_sub).  window_hot_sub keeps governing ratings only.  Set before the data set is built:
 *                                                               train_dataset refuses a sequence built with another window_pair_sub.  Refused with amd:contrib = bf16,
 *                                                               user-group trainers, amd:gpus > 1, svdf_dataset_window_from_pairs, num_factor > 256 ("window_pair_sub > 0 needs
 *                                                               num_factor <= 256": the pair lane has no wide rows).  Calibration: profiles/r12_pair_hot.md
 *     ipc_spin_limit             polls before a flag wait of the IPC exchange gives up
 *     rank_eval_budget 4194304   svdf_rank_eval_positions: positives + distinct banned ids + sections processed per piece of whole sections (>= 1)
 *     rank_topn_budget 33554432  svdf_rank_topn: 64-bit keys (8 bytes each) of the selection's list workspace; a call that needs more takes fewer
 *                                item ranges per section first, then pieces of whole sections (>= 1; results do not depend on it)
 *     pair_hard_form      0      the kernel of a hard pass of a pair source (svdf_dataset_from_pair_source_hard): 0 the measured
 *                                choice (the staged form up to num_cand 16 at num_factor <= 32, up to 4 at <= 128, for 2 at <= 256, the lane form
 *                                otherwise; profiles/r34_pair_hard.md), 1 one lane per candidate with both rows read where they lie, 2 the item
 *                                rows staged in the wave's LDS (num_factor > 256 always takes 1).  Same bits
 *     pair_weight_form    0      the map of a draw from a pair source with item weights (svdf_pair_source_create_weighted): 0 the
 *                                measured choice (2 up to 10 000 items, 1 above; profiles/r36_pair_weight.md), 1 a binary search of the whole
 *                                table of running sums, 2 a guide table indexed by the word's high bits, then a search between two of its
 *                                entries.  Same bits
 * Returns 0 if the knob exists, -1 otherwise.  The relaxed mode is switched by CONFIG keys through svdf_set_param ("amd:relax_global",
 * "amd:relax_user_from", "amd:relax_item_from", "amd:relax_feedback"), not by knobs: it changes results.  So is
 * "amd:shared_user_from" = B (one GPU, the window step of amd:step = minibatch / auto): user ids < B are private (exactly one
 * per row, walked exactly), ids >= B are shared attribute rows (any number per row, read as of the window start and moved once per window
 * like item rows).  1 <= B <= num_user; refused with amd:gpus > 1, amd:contrib = bf16 and in svdf_dataset_window_from_csr.
 * On a user-group (format_type 1, SVD++) trainer every row of a DEFAULT block or START..END span carries the same private id
 * -- the unit's user -- and any number of shared ids, which may differ from row to row (user-side attributes: region, device class, social
 * group).  They join tmp_ufactor and calc_bias in entry order on top of the feedback state, and move once per window like item and feedback
 * rows.  Reached under amd:step = minibatch from svdf_dataset_from_blocks and svdf_dataset_from_buffer_file(.., 1); scored by
 * svdf_predict_dataset / svdf_eval_dataset.  The window step's accuracy contract has not been measured on such blocks
 * (profiles/r15_block_shared.md); until it has, `auto` (decision 3) and the staged svdf_update_block route (counter 31, the one stderr line)
 * keep blocks with shared ids on the exact pass.  Refused there as well: a span whose rows name two private ids; in
 * svdf_dataset_window_from_blocks a row with several user entries of which one is >= B (a row whose ONLY user entry is >= B is an ordinary
 * user to that entry point, as without the key); side tables and the ordered sub-step lanes of the other routes (window_shared_sub,
 * window_item_sub, window_pair_sub) stay refused with user-group trainers -- hot shared rows of such blocks have a lane of their own, knob
 * window_block_sub, and so have their hot item rows, knob window_block_item_sub (it does not need this key).
 * Blocks whose rows have one user entry < B train bit for bit as without the key (in the window sequence a row whose only user entry is >= B
 * has no private id and is refused). */
int svdf_set_knob(svdf_trainer *t, const char *name, long value);

/* ---- evaluation: RMSEEvaluator of svd_feature_infer.cpp:38-56,243-277 over a resident data set.  Predictions
 * stay in HBM; *sum_sq_err = sum over instances of ((pred - label) * scale_score)^2 (difference and scaling in fp32, square and
 * sum in fp64 like add_eval), *count = instances; RMSE = sqrt(sum / count) (print_stat).  The sum is a fixed fp64 tree on the
 * device + long double over the partial sums, the reference's is a sequential long double sum: equal to ~1e-13 relative.
 * Works on the data sets of an "amd:gpus" handle (every piece is scored on the rank that holds it; svdf_predict_dataset refuses those:
 * their rows are regrouped, there is no file order to report predictions in) and on window data sets: a window sequence is scored window by
 * window, the partial sums of all windows added on the host; rank-pair windows carry label 1 for every pair (apex_svd_data.cpp:905-911); a
 * stand-alone window trained but not yet applied is scored against the model without its pending sums (see svdf_predict_dataset). */
int svdf_eval_dataset(svdf_trainer *t, svdf_dataset *ds, float scale_score, double *sum_sq_err, int64_t *count);

/* ---- ranking: class apex_svd::ISVDRanker (apex_svd.h:160-197) as implemented by SVDFeatureRanker
 * (solvers/base-solver/apex_svd_base.h:597-813), obtained from create_svd_ranker(SVDTypeParam) (apex_svd.h:222).
 *   svdf_ranker_set_param   ISVDRanker::set_param: feature_user, feature_item, top_k (:656-660)
 *   svdf_ranker_load_model  ISVDRanker::load_model (:662-664); the caller has consumed the 4-byte SVDTypeParam
 *   svdf_ranker_init        ISVDRanker::init_ranker(num_item_set) (:666-685)
 *   svdf_ranker_process_*   ISVDRanker::process(std::vector<int>&, Elem / SVDPlusBlock) (:797-812): the tag travels in the
 *                           label field (svdranker_tag, apex_svd.h:115-152: 0 ITEM, 2 USER, 1 POS, -1 BAN, 3 SPEC, 4 PROCESS).
 *                           Results of the line (top_k item indices, or the rank positions of the positive samples) are
 *                           written to out[0..capacity); the return value is the number of results (may exceed capacity:
 *                           call again with a larger buffer is NOT possible, size it num_item_set), -1 on error.
 * Scores are computed on the GPU in the reference's fp32 order; the results are the reference's, index for index. */
svdf_ranker *svdf_ranker_create(uint8_t format_type, uint8_t active_type, uint8_t extend_type, uint8_t variant_type, int device);
void svdf_ranker_destroy(svdf_ranker *r);
int svdf_ranker_set_param(svdf_ranker *r, const char *name, const char *val);
int svdf_ranker_load_model(svdf_ranker *r, FILE *fi);
int svdf_ranker_init(svdf_ranker *r, int num_item_set);
int64_t svdf_ranker_process_csr(svdf_ranker *r, float label, int num_global, int num_ufactor, int num_ifactor, const unsigned *index,
                                const float *value, int *out, int64_t capacity);
/* Bulk form: the rank task's loop over a whole CSR input (svd_feature_infer.cpp:347-375: every line of the iterator goes through
 * process(), results appended) in ONE call.  Same results in the same order as num_row calls of svdf_ranker_process_csr; user
 * sections are pipelined on the device (up to 8 in flight), so a section costs its enqueue, not a launch + sync round trip. */
int64_t svdf_ranker_process_rows(svdf_ranker *r, int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index,
                                 const float *feat_value, int *out, int64_t capacity);
int64_t svdf_ranker_process_block(svdf_ranker *r, int num_ufeedback, int extend_tag, const unsigned *index_ufeedback,
                                  const float *value_ufeedback, int num_row, const float *row_label, const int *row_ptr,
                                  const unsigned *feat_index, const float *feat_value, int *out, int64_t capacity);
/* counters: 0 user sections ranked, 1 sections finished by the host sort because scores tied at a requested position,
 * 2 positive samples of the open user section (what a PROCESS line would report now when top_k = 0: sizes the output) */
int64_t svdf_ranker_counter(svdf_ranker *r, int what);

/* ---- batch ranking evaluation on the LIVE model: where the positives a user held out rank among ALL items, for many
 * users in one call, and the reference's ranking metrics (apex-utils/apex_evaluator.h:33-215) of those positions.  No model file, no
 * second handle, no candidate matrix: the sweep reads W_item where the trainer keeps it.
 *
 * A format_type = 0, extend_type = 0 trainer with its model in HBM.  Section s of S: the user user[s], its held-out positives
 * pos_item[pos_ptr[s] .. pos_ptr[s + 1]) and its banned items ban_item[ban_ptr[s] .. ban_ptr[s + 1]) -- the user's training items;
 * ban_ptr == NULL: none.  The candidates of every section are the item ids 0 .. num_item - 1; a candidate is RANKED unless it is banned,
 * positives are ranked candidates like any other.  The score of candidate i is proc_rank's (apex_svd_base.h:754-765) for a USER line
 * user[s]:1 and ITEM lines i:1: i_bias[i] + <W_user[user[s]], W_item[i]> in the ranker's fp32 order, bit for bit what svdf_ranker_*
 * computes from the saved model (no user bias, no base score, no link).  For positive p (entry j of pos_item):
 *   position_out[j] = ranked candidates scoring strictly higher than p + ranked candidates c != p with score_c == score_p and c < p
 *   tied_out[j]     = ranked candidates c != p with score_c == score_p
 * +0 and -0 compare equal.  The reference shuffles before it sorts (apex_evaluator.h:178), so its order inside a tie is random; here a
 * tie is broken by item id, and tied_out says where that happened (tied == 0: the position is the ranker's, index for index).
 *   ranked_out[s]   = num_item - distinct banned ids of the section
 *   nan_out[s]      = 1 when a ranked candidate (a positive included) scores NaN: the section's positions are -1, the metrics skip it
 * Duplicate ban ids count once.  Refused, with the ranker's messages: a positive that is also banned ("each pos sample item can not occur
 * in baned sample list"), ids out of range ("user feature index exceed bound", "sample item index exceed bound"); a positive repeated
 * inside a section.  A section without positives returns nothing.  A user may appear in several sections.  Everything is validated on
 * the host before any device work.  The call runs on the trainer's stream behind the passes already queued and returns when the results
 * are on the host; a stand-alone window trained but not yet applied is ranked against the model without its pending sums (see
 * svdf_predict_dataset).  Lists of more than `rank_eval_budget` entries (knob, default 4194304 positives + distinct bans + sections) are
 * processed in pieces of whole sections.  Counter 38 counts the sections ranked.
 * Refused, each with its cause: user-group trainers and extend_type != 0, feature_user / feature_item side tables (they change the
 * score), common_latent_space != 0, amd:gpus > 1 and the per-rank handles of the exchange schemes, host-only handles ("needs a GPU").
 * svdf_ranker_* remains the route for those.
 *
 * svdf_rank_eval_metrics is a host function (no GPU, no handle): sections [sec_ptr[s], sec_ptr[s + 1]) of position[], each sorted ascending
 * first (add_eval(pos_idx, false)), then added in section order in double precision exactly as EvaluatorMAP::add_eval / print_result do
 * -- MAP sum_i (i + 1) / (pos_i + 1) / npos; MAP@k, Pre@k, Rec@k with the counter j of :146-166 and the FLOAT running sum sum_ar of
 * :138-142 -- for up to 8 cut-offs, handled in ascending order (out->at).  The figures the reference prints are sum / ninst.  Empty
 * sections and sections with nan[s] != 0 (nan may be NULL) are no instances: they count under skipped / nan_sections.  With ranked != NULL
 * a per-section AUC, which is NOT in the reference, is added too: positives sorted, 0-based,
 * AUC_s = 1 - sum_i (pos_i - i) / ((double)npos * (double)(ranked[s] - npos)), left out when ranked[s] == npos (nauc counts the rest).
 * Positions from svdf_ranker_process_* can be fed as well.  svdf_rank_eval does both steps. */
typedef struct svdf_rank_metrics {
    int64_t ninst, skipped, nan_sections, nauc;
    int num_at, at[8];                 /* the cut-offs, ascending */
    double sum_map, sum_map_at[8], sum_pre_at[8], sum_rec_at[8], sum_auc;
} svdf_rank_metrics;
int svdf_rank_eval_positions(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item,
                             const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out);
int svdf_rank_eval_metrics(long num_section, const int64_t *sec_ptr, const int *position, const int *ranked, const int *nan, int num_at,
                           const int *at, svdf_rank_metrics *out);
int svdf_rank_eval(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item,
                   const int64_t *ban_ptr, const unsigned *ban_item, int num_at, const int *at, svdf_rank_metrics *out);

/* ---- top-N item lists on the live model: the other half of ISVDRanker -- top_k -- for many users in one call, on
 * the trainer's own model: which items do we recommend?  The preconditions are svdf_rank_eval_positions': a format_type = 0,
 * extend_type = 0 trainer with its model in HBM; refused, each with its cause and in the same words behind the prefix "rank_topn:", are
 * user-group trainers and extend_type != 0, feature_user / feature_item side tables, common_latent_space != 0, amd:gpus > 1 and the
 * per-rank handles of the exchange schemes, and host-only handles ("needs a GPU", raised after the lists have been validated).
 *
 * Section s of num_section: the user user[s] with the banned items ban_item[ban_ptr[s] .. ban_ptr[s + 1]); ban_ptr == NULL: no section has
 * bans.  Duplicate ban ids count once.  The candidates are all item ids 0 .. num_item - 1; a candidate is RANKED unless it is banned.  Its
 * score is svdf_rank_eval_positions': 0 + (i_bias[i] + <W_user[user[s]], W_item[i]>) in the ranker's fp32 order (four chains over the
 * 4-float chunks, (a0 + a2) + (a1 + a3), the scalar tail, bias + sum; no FMA), bit for bit what svdf_ranker_* computes from the saved model.
 * ORDER: higher score first; equal scores by ASCENDING ITEM ID; +0 == -0.  The reference's std::sort (apex_svd_base.h:767) leaves the order
 * inside a tie unspecified; here it is by id, the rule of svdf_rank_eval_positions, so position r of that call is entry r of this one.
 *   count_out[s]              = min(top_n, num_item - distinct banned ids): the reference asserts "k can not exceed candidate size", the
 *                               batch call returns the shorter list
 *   item_out[s * top_n + r]   = the id at rank r for r < count_out[s], -1 beyond
 *   score_out[s * top_n + r]  = that item's score, 0.0f beyond; score_out may be NULL
 *   nan_out[s]                = 1 when a RANKED candidate scores NaN: the section's whole list is -1 / 0.0f and count_out[s] = 0 (a banned
 *                               NaN row does not flag)
 * 1 <= top_n <= 256; a larger top_n is refused ("top_n must be between 1 and 256"): rank the saved model with svdf_ranker_* and top_k.
 * Ids out of range are refused with the ranker's messages ("user feature index exceed bound", "sample item index exceed bound"); all
 * validation runs on the host before any device work.  num_section == 0 returns 0 and launches nothing.  A user may appear in several
 * sections.  The call runs on the trainer's stream behind whatever is queued and returns when the results are on the host; a stand-alone
 * window trained but not yet applied is ranked without its pending sums (see svdf_predict_dataset).  The per-(section, item range) lists of
 * the selection live in a device workspace of at most `rank_topn_budget` 64-bit keys (knob, default 33554432 = 256 MiB): fewer item ranges
 * first, then pieces of whole sections; the result does not depend on the knob.  Counter 39 counts the sections listed. */
int svdf_rank_topn(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n,
                   int *item_out, float *score_out, int *count_out, int *nan_out);

/* ---- the two calls above for USER-GROUP (format_type = 1, SVD++) trainers: sections with feedback lists.  Each _fb
 * entry point is its twin plus three arguments behind `user`: section s carries the feedback list fb_index / fb_value[fb_ptr[s] ..
 * fb_ptr[s + 1]) of (id, value) pairs, in the order in which the reference's ranker would add them.  The score of candidate i is the
 * ranker's for one block holding that list, a USER line user[s]:1 and ITEM lines i:1 (apex_svd_base.h:719-735, 798-808):
 *   tmp_ufeedback = 0;  for j in list order:  tmp_ufeedback += W_ufeedback[fb_index[j]] * fb_value[j]
 *   tmp_ufactor   = tmp_ufeedback;            tmp_ufactor   += W_user[user[s]] * 1
 *   score(i)      = 0 + (i_bias[i] + <tmp_ufactor, W_item[i]>)                     -- the dot product in the order given above
 * every multiply and add rounded separately to fp32 (no FMA), a value within 1e-6 of 1 multiplying as exactly 1 (the reference's
 * scalar_map): bit for bit what svdf_ranker_process_block computes from the saved model.  A list's sum is a serial chain per element in
 * list order; it is never split or reassociated, so a long list costs its length.  Everything else is the twin's, unchanged:
 * positives, bans, ties by id, +-0, count, top_n <= 256, pieces, outputs, and "validated on the host before any device work, and before
 * `needs a GPU`".
 * Accepted: format_type = 1 trainers with extend_type 0 or 1 (both are SVDPPFeature with one model).  LEGAL: an empty list (the row is
 * 0 + W_user[u] * 1); an id repeated inside a list (added twice, in order); any float value; a user in several sections with different
 * lists.  A NaN that reaches a row through a value (or through W_ufeedback) flags the section like any NaN score.  A NaN VALUE is the
 * one input on which the call leaves the ranker: the reference's scalar_map takes a NaN scalar for 1 (its |s - 1| > 1e-6 test is false) and
 * adds the row unscaled; here the NaN reaches every element of the section's row and flags the section.
 * REFUSED on the host, behind the prefixes "rank_eval:" / "rank_topn:" (the ranker's message bare):
 *   a feedback id >= num_ufeedback                     "ufeedback id exceed bound"
 *   fb_ptr that starts below 0 / decreases             "fb_ptr must start at >= 0" / "fb_ptr must not decrease"
 *   entries without fb_index or fb_value               "fb_index / fb_value is missing"
 *   fb_ptr == NULL on a user-group trainer             "fb_ptr is NULL on a user-group trainer; a section without feedback must be given
 *                                                      explicitly as an empty list ..." -- the reference's ranker scores such a section
 *                                                      with a clone of W_user[0] left over from init_ranker (:680-682), an accident the
 *                                                      batch call does not reproduce
 *   fb_ptr != NULL on a format_type = 0 trainer        "feedback lists need a user-group trainer"
 *   extend_type 2 / 15, feature_user / feature_item side tables, common_latent_space != 0, amd:gpus > 1, rank handles: as the twins do,
 *   in the same words.
 * On a format_type = 0 trainer a _fb call with fb_ptr == NULL IS the twin.  The twins themselves are unchanged: they refuse user-group
 * trainers as before.
 * Per piece the lists ride in the piece's one upload and one more kernel launch (k_rank_live_rows) builds the sections' rows into a
 * workspace of sections x pitch floats, which the sweeps read instead of W_user rows.  Feedback entries count towards `rank_eval_budget`
 * in the evaluation call; the top-N call also ends a piece whose feedback entries would exceed that knob.  No result depends on a knob.
 * Counter 40 counts the sections ranked with a row built from a feedback list: of the sections counters 38 / 39 count (which count as
 * before), those of _fb calls on user-group trainers. */
int svdf_rank_eval_positions_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index,
                                const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                                const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out);
int svdf_rank_eval_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                      const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_at, const int *at,
                      svdf_rank_metrics *out);
int svdf_rank_topn_fb(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                      const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out);

/* ---- the same calls for sections that bring a USER LINE, and for trainers with feature_user / feature_item SIDE TABLES (DESIGN.md section
 * 6z).  Each _lines entry point is its _fb twin with `user` replaced by a USER line per section: section s carries the (id, value) entries
 * ul_index / ul_value[ul_ptr[s] .. ul_ptr[s + 1]) in line order -- a user id plus attribute ids, say.  The feedback triple, the positives, the
 * bans and every output keep their _fb meaning, order and types.  The score of candidate i is the ranker's for that USER line and ITEM
 * lines i:1 (proc_user / prepare_ifactor, apex_svd_base.h:687-735), with the trainer's side tables:
 *   tu = 0 (format_type = 0), or 0 + sum_j W_ufeedback[fb_index[j]] * fb_value[j] in list order (a user-group trainer, section 6y's chain)
 *   for each entry j of the line, in line order:   tu += W_user[uid_j] * val_j
 *       then, if uid_j < the feature_user table's rows, for each child c of uid_j in table order:   tu += W_user[cid_c] * cval_c
 *   -- the child is NOT scaled by val_j, and children of children are not followed: both are the reference's behaviour (:731-734).
 *   With a feature_item table the item side is prepared once per call, for every item i:
 *       f = 0;  f += W_item[i] * 1;  per child c of i in table order:  f += W_item[cid_c] * (float)((double)cval_c * 1.0)
 *       b = 0 + i_bias[i] * 1;       per child:                        b = b + i_bias[cid_c] * cval_c * 1
 *   (ids at or past a table's row count have no children); without one the sweeps read W_item / i_bias in place, exactly as the twins do.
 *   score(i) = 0 + (b_i + <tu, f_i>) -- the dot product in the order given above.
 * Every multiply and add is rounded separately to fp32 (no FMA), a value within 1e-6 of 1 multiplying as exactly 1 (scalar_map); a line's
 * sum is a serial chain per element in line order, never split or reassociated.  Everything behind the two rows is svdf_rank_eval_positions'
 * and svdf_rank_topn's, bit for bit: positions, tied, keys, the order of a list, NaN flagging, count, top_n <= 256, duplicate bans.
 * LEGAL: an empty line (the row is the feedback sum, or 0); an id repeated inside a line (added twice, with its children twice); any float
 * value; a child equal to its parent.  A NaN VALUE in a line is treated as section 6y treats a NaN feedback value: it reaches every element
 * of the section's row and flags the section (the reference's scalar_map would take it for 1).  A NaN that reaches a row through the
 * model or a table value flags like any NaN score.
 * ACCEPTED: format_type = 0 trainers with extend_type = 0 (fb_ptr must be NULL); format_type = 1 trainers with extend_type 0 or 1 (fb_ptr is
 * required, as in section 6y); each with or without either side table.
 * REFUSED in the twins' words behind the prefixes "rank_eval:" / "rank_topn:": extend_type 2 / 15, common_latent_space != 0, amd:gpus > 1,
 * rank handles, host-only handles ("needs a GPU").  REFUSED on the host, before any device work and before "needs a GPU":
 *   a line id >= num_user                              "user feature index exceed bound" (the ranker's message, bare)
 *   ul_ptr NULL / starting below 0 / decreasing        "ul_ptr is missing" / "ul_ptr must start at >= 0" / "ul_ptr must not decrease"
 *   entries without ul_index or ul_value               "ul_index / ul_value is missing"
 *   a side-table child id outside its id space         "feature_user: child index exceed bound" / "feature_item: ..." (the table loader
 *                                                      refuses it at init_trainer too; the calls check once more, the tables are small)
 *   and everything the _fb twins refuse about feedback lists, positives and bans, in their words.
 * num_section == 0 launches nothing.  The six entry points above do not change: they still refuse side tables.
 * Per piece the lines ride in the piece's one upload and k_rank_live_rows builds the sections' rows (one launch, as in section 6y).  With a
 * feature_item table one more launch per CALL (k_rank_live_items) prepares the item matrix and bias vector into a workspace of
 * num_item * (pitch + 1) * 4 bytes on the trainer's stream ahead of the sweeps; an allocation failure names that size.  The matrix is not
 * kept across calls.  Line entries count towards `rank_eval_budget` like feedback entries; no result depends on a knob.
 * Counter 41 counts, of the sections under counters 38 / 39, those ranked with a row built from a USER line, i.e. those of the _lines
 * calls.  Counters 38 - 40 count as before (40: the sections whose row holds a feedback sum, _lines calls on user-group trainers included). */
int svdf_rank_eval_positions_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                                   const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                   const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out,
                                   int *ranked_out, int *nan_out);
int svdf_rank_eval_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value, const int64_t *fb_ptr,
                         const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                         const unsigned *ban_item, int num_at, const int *at, svdf_rank_metrics *out);
int svdf_rank_topn_lines(svdf_trainer *t, long num_section, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value, const int64_t *fb_ptr,
                         const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out,
                         float *score_out, int *count_out, int *nan_out);

/* ---- the same rankings over PER-SECTION CANDIDATE LISTS: section s ranks over an item set the caller defines,
 * cand_item[cand_ptr[s] .. cand_ptr[s + 1]), not over 0 .. num_item - 1 minus a ban list -- the reference's SVDFeatureRanker over the ITEM
 * lines of a section (apex_svd_base.h:711-782).  Sampled-negative evaluation (a held-out positive among 99 or 999 sampled negatives) and
 * re-ranking a retrieved shortlist are these calls.  Only the listed (section, item) pairs are scored; a pair costs one gathered item row.
 * WHO THE SECTION IS: exactly one of `user` / `ul_ptr` is non-NULL ("give the sections either as users or as USER lines" otherwise).
 *   user:    the section's row is svdf_rank_eval_positions' (the W_user row in place); on a user-group trainer section 6y's (the feedback
 *            chain + W_user[u] * 1; fb_ptr is required there and must be NULL on a format_type = 0 trainer).  Side tables are refused in the
 *            twins' words.
 *   ul_ptr:  the section's row is section 6z's (a USER line of (id, value) entries, feature_user children, behind the feedback chain on a
 *            user-group trainer); the trainer may have feature_user / feature_item side tables.
 * The accepted and refused configurations are otherwise those of the matching twin (_fb with `user`, _lines with `ul_ptr`), in its words.
 * WHAT IS RANKED: there are no bans -- a caller leaves out what must not be ranked.  For the positions calls the ranked set of section s is
 * the DISTINCT ids of its candidate list together with the section's positives: a positive is a candidate by definition, and listing it
 * among the candidates as well counts it once.  For the top-N call it is the distinct ids of the list alone.  Duplicate ids count once, as
 * duplicate bans do.
 * SCORE: exactly the score the twin gives that (section, item) pair, the same operations in the same order -- four serial chains over the
 * 4-float chunks, (a0 + a2) + (a1 + a3), the scalar tail, 0 + (bias + sum), every multiply and add rounded separately to fp32; with a
 * feature_item table the prepared item row and bias of section 6z.  It is bit for bit what svdf_ranker_* gives on the saved model.
 * OUTPUTS: position_out / tied_out [pos_ptr[num_section]]: the twins' definition over the ranked set -- position = candidates that score
 *   strictly higher + tied ones with a smaller id; tied = other candidates with an equal score; +0 == -0, NaN equals nothing.
 *   ranked_out[s]: the size of the ranked set.  nan_out[s]: 1 when a RANKED candidate scores NaN (a NaN row of an item outside the
 *   section's set does not flag); the section's positions and tied are then -1, or its list is empty with count_out[s] = 0.
 *   item_out / score_out [num_section][top_n], count_out [num_section]: svdf_rank_topn's layout, count_out[s] = min(top_n, distinct
 *   candidates); higher score first, equal scores by ascending id; -1 / 0 beyond count_out[s].  1 <= top_n <= 256.  score_out may be NULL.
 * LEGAL: an empty candidate list (with positives: their positions among themselves; top-N: count_out = 0); a user in several sections with
 * different lists; a list that covers the whole catalogue; a section without positives (ranked_out is filled, nothing of it is scored).
 * REFUSED on the host, before any device work and before "needs a GPU", behind the prefix "rank_eval:" / "rank_topn:":
 *   a candidate id >= num_item                           "sample item index exceed bound" (the ranker's message, bare)
 *   cand_ptr NULL / starting below 0 / decreasing        "cand_ptr is missing" / "cand_ptr must start at >= 0" / "cand_ptr must not decrease"
 *   entries without cand_item                            "cand_item is missing"
 *   a positive repeated inside a section                 "rank_eval: a positive item is repeated inside a section"
 *   and everything the twins refuse about users, lines, feedback lists, positives and top_n, in their words.
 * num_section == 0 launches nothing; a positions call without any positive launches nothing.
 * A call is cut into pieces of whole sections whose entries (candidate pairs, positives, feedback and line entries, one per section) stay
 * within the knob `rank_eval_budget`, in both kinds of call; a section larger than the budget is a piece of its own.  Per piece: one upload
 * (the deduplicated lists in ascending id order, the tile table, the rows' lists), the workspaces cand_score (4 bytes per pair) and the
 * results; an allocation failure names the size.  No result depends on a knob (`rank_cand_form`: 0 the measured choice of the score kernel's
 * form, 1 one lane per pair, 2 staged in LDS).  With a feature_item table the whole catalogue is still prepared once per call.
 * Counter 42 counts the sections ranked over a candidate list; they count under 38 (positions: sections with positives) / 39 (top-N) too,
 * and under 40 / 41 as the twins' do.  The nine entry points above do not change. */
int svdf_rank_eval_positions_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                                  const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                  const unsigned *pos_item, const int64_t *cand_ptr, const unsigned *cand_item, int *position_out, int *tied_out,
                                  int *ranked_out, int *nan_out);
int svdf_rank_eval_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                        const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr, const unsigned *pos_item,
                        const int64_t *cand_ptr, const unsigned *cand_item, int num_at, const int *at, svdf_rank_metrics *out);
int svdf_rank_topn_cand(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index, const float *ul_value,
                        const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *cand_ptr, const unsigned *cand_item,
                        int top_n, int *item_out, float *score_out, int *count_out, int *nan_out);

/* ---- the positions calls against negatives the DEVICE draws: sampled-negative evaluation -- held-out positives
 * ranked among num_neg items the user has not interacted with -- without candidate lists on the host.  The caller hands over what the
 * full-catalogue calls take (users or USER lines, feedback lists, positives, bans = the users' training items) and two scalars.
 * THE RULE, pure 64-bit unsigned integer arithmetic, wrapping mod 2^64:
 *   G         = 0x9E3779B97F4A7C15
 *   mix(z)    : z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   stream_s  = mix(seed + (s + 1) * G)                       s: the section's index IN THE CALL (never in a piece of it)
 *   draw(s,t) = (uint32)(((mix(stream_s + (t + 1) * G) >> 32) * (uint64)num_item) >> 32)       t = 0, 1, 2, ...
 * -- splitmix64 seeded per section from a splitmix64 of the seed, mapped onto an id by multiply-high; the bias of at most num_item / 2^32
 * is accepted.  excluded_s is the distinct ids of the section's bans together with its positives.  THE NEGATIVES of section s are the
 * first num_neg ids of the sequence draw(s, 0), draw(s, 1), ... that are not in excluded_s and have not occurred earlier in the sequence;
 * they keep the order of the sequence.  THE RANKED SET is the section's positives plus its negatives; over it everything is
 * svdf_rank_eval_positions_cand's: position, tied, ties by ascending id, +0 == -0, nan_out set only by a RANKED candidate, the score of a
 * pair the twin's bit for bit; ranked_out[s] = npos_s + num_neg.  A section without positives is not drawn or scored: ranked_out[s] =
 * num_neg, its neg_out row is -1, its ids are still validated.
 * PINNED VECTORS (seed 12345, num_item 1200): stream_0 = 0x22118258a9d111a0, stream_7 = 0x6e7411b06820371c;
 *   section 0, nothing excluded, draws t = 0 .. 5:  18, 601, 213, 846, 111, 362
 *   section 7, excluded {25, 303}, draws t = 0 .. 7: 1196, 25, 1196, 303, 504, 615, 588, 726 (the third repeats the first);
 *              its num_neg = 5 negatives are 1196, 504, 615, 588, 726, after 8 draws.
 * WHO THE SECTION IS: exactly the _cand calls' rule -- one of `user` / `ul_ptr`, fb_ptr on user-group trainers, side tables only with
 * lines; the configurations the twins refuse are refused in their words.  BANS AND POSITIVES are validated as svdf_rank_eval_positions
 * validates them (range, the shape of ban_ptr, "each pos sample item can not occur in baned sample list", a repeated positive); ban_ptr ==
 * NULL: no bans.  REFUSED besides, on the host, before any device work and before "needs a GPU":
 *   num_neg outside 1 .. 4096                            "rank_eval: num_neg must be between 1 and 4096"
 *   a section WITH positives that leaves avail = num_item - |excluded_s| ids with avail < 2 * num_neg or avail * 64 < num_item
 *       "rank_eval: section S leaves A items to draw NUM_NEG negatives from NUM_ITEM; list its candidates instead (svdf_rank_eval_positions_cand)"
 * -- the two conditions make every draw succeed with probability >= 1 / 128, so a section expects at most 128 * num_neg draws and no
 * input makes the kernel run long.
 * neg_out [num_section][num_neg], or NULL: the negatives in draw order.  num_section == 0 and a call without any positive launch nothing.
 * Pieces of whole sections within the knob `rank_eval_budget` (entries: pairs, positives, excluded ids, feedback and line entries, one per
 * section); no result depends on a knob or on the pieces.  Per piece one upload of the small tables, the positives, the excluded lists
 * and the rows' lists; the candidate ids are a device workspace that k_rank_negs_draw (a wave per section) fills.  An allocation failure
 * names the size.  Counter 43 counts the sections ranked against drawn negatives; they count under 38, and under 40 / 41 as the twins' do,
 * not under 42.  The entry points above do not change.
 * svdf_rank_negatives is the rule on the host -- no GPU, no handle: the same validation and refusals, neg_out as above. */
int svdf_rank_negatives(long num_section, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item,
                        long num_item, int num_neg, uint64_t seed, int *neg_out);
int svdf_rank_eval_positions_sampled(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                                     const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                     const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg,
                                     uint64_t seed, int *position_out, int *tied_out, int *ranked_out, int *nan_out, int *neg_out);
int svdf_rank_eval_sampled(svdf_trainer *t, long num_section, const unsigned *user, const int64_t *ul_ptr, const unsigned *ul_index,
                           const float *ul_value, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                           const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg, uint64_t seed, int num_at,
                           const int *at, svdf_rank_metrics *out);

/* ---- passes of rank pairs from POSITIVES ONLY, the negatives drawn on the device.  Pairwise training on implicit
 * feedback needs a fresh negative per positive every round; svdf_dataset_from_pairs takes three finished columns, so its caller draws and
 * uploads them every round.  A pair source keeps the positives in HBM -- one upload at creation, nothing per pass -- and a pass is two scalars.
 * THE RULE, pure 64-bit unsigned integer arithmetic, wrapping mod 2^64; G, mix and the map onto an id are the sampled calls' above:
 *   a source has rows r = 0 .. n-1 of (user_r, pos_r), in the caller's order; P(u) = the distinct items of ALL rows of user u
 *   a pass has num_neg = m negatives per row: pair q = r * m + j (j = 0 .. m-1) is (user_r, pos_r, neg_q) -- the m pairs of a row are
 *   adjacent, rows stay in source order
 *   SALT      = 0x70616972736E6567      (ASCII "pairsneg": a pass and a sampled evaluation with one seed draw from different streams)
 *   stream_q  = mix((seed ^ SALT) + (q + 1) * G)
 *   draw(q,t) = (uint32)(((mix(stream_q + (t + 1) * G) >> 32) * (uint64)num_item) >> 32)       t = 0, 1, 2, ...
 *   neg_q     = the first of draw(q, 0), draw(q, 1), ... that is not in P(user_r)
 * The m negatives of a row are independent (repeats among them are allowed); pos != neg holds by construction.  AT MOST T = 4096 DRAWS per
 * pair: a pair that exhausts them fails the call ("pair_source: pair Q found no negative in 4096 draws") and never loops further.  A source
 * is refused when a user with rows has 64 * (num_item - |P(u)|) < num_item; every source that remains accepts each draw with probability
 * >= 1 / 64, so a pair exceeds T with probability <= (63 / 64)^4096 = exp(4096 * ln(63 / 64)) < exp(-64.5) < 1e-28.
 * PINNED VECTORS (seed 12345, num_item 1200): stream_0 = 0x6df61f806828913e, stream_7 = 0x0cee3333c9e3d7d8;
 *   pair 0, draws t = 0 .. 5: 607, 1083, 476, 1017, 945, 510;   pair 7, draws t = 0 .. 7: 496, 554, 32, 921, 199, 15, 1103, 184
 *   rows (user, pos) = (4, 10), (4, 700), (9, 10): num_neg 1 gives the negatives 607, 549, 766; num_neg 2 gives 607, 549, 766, 1010, 64, 448
 *   a pair 0 whose user has 607 among its positives takes 1083, its second draw.
 * REFUSED on the host, before any device work and before "needs a GPU" (a host-only handle creates sources and reaches every message):
 *   at creation   n < 1                                     "pair_source: a source needs at least one row (n >= 1)"
 *                 an id out of range, row by row            "user feature index exceed bound" / "item feature index exceed bound"
 *                 the density rule                          "pair_source: user U has D distinct positive items of NUM_ITEM: fewer than 1 item
 *                                                            in 64 is left to draw a negative from; draw its negatives yourself (svdf_dataset_from_pairs)"
 *                 before init_trainer                       "pair_source: call init_model / load_model and init_trainer first"
 *   per pass      a source of another trainer (or of one that is gone)   "pair_source: the source was created on another trainer"
 *                 num_neg outside 1 .. 256                  "pair_source: num_neg must be between 1 and 256"
 *                 n * num_neg >= 2^31 - 16                  "pair_source: n * num_neg must stay below 2^31 - 16"
 * -- and what svdf_dataset_from_pairs refuses about the trainer, in its words.
 * svdf_dataset_from_pair_source draws the pass's three columns (n * num_neg entries each) in HBM with one launch of k_pair_draw, a lane
 * per pair, and returns the data set svdf_dataset_from_pairs returns for those columns -- the same kind, the same schedule or windows, the
 * same trained bits.  The columns stay in HBM (counter 44) where that builder has a form that starts from device columns: under `amd:step =
 * minibatch` on one GPU with the device window builder and window_pair_sub = 0 (the window sequence, built as section 6v builds it), and on
 * the exact pass where it schedules on the device and the expanded user column is not user-grouped (user-run units are built on the host).
 * "User-grouped" is svdf_dataset_from_pairs' own pretest, at least half of the adjacent pairs sharing their user; the num_neg pairs of a row
 * are adjacent, so with num_neg >= 2 the expanded column always is.  With the default knobs the exact pass therefore stays in HBM for
 * num_neg = 1 on a source that is not user-grouped, and only there; num_neg >= 2 stays in HBM on the exact pass only with pair_units = 0.
 * Everywhere else -- `amd:step = auto`, amd:gpus > 1, relaxed ids, side tables, lazy decay, wide rows, window_pair_sub > 0, user-grouped
 * orders, user-group trainers -- the columns are copied back and svdf_dataset_from_pairs builds from them (counter 45).  No result
 * depends on the route.  An allocation failure names the size.
 * svdf_pair_source_draw copies the negative column the device draws to neg_out[n * num_neg]; svdf_pair_negatives is the rule on the host --
 * no GPU, no handle -- with the same validation.  svdf_pair_source_destroy is also valid after svdf_destroy of the source's trainer; data
 * sets built from a source do not refer to it.  No older entry point changes.
 * MEASURED (one MI355X, 100 K users x 10 K items, 20 M shuffled positives, num_factor 128, num_neg 1; medians of five rounds of build +
 * train + synchronize + destroy; profiles/r33_pair_source.md): 0.280 s per round on the exact pass, 0.149 s under `amd:step = minibatch`,
 * against 2.52 s / 2.34 s for svdf_pair_negatives on the host followed by svdf_dataset_from_pairs, whose draw alone takes 2.1 .. 2.3 s;
 * k_pair_draw takes 1.4 ms.  On columns that are drawn already the exact pass gains nothing from the source.  Not measured: num_neg > 1,
 * user-grouped orders, the fallback configurations. */
svdf_pair_source *svdf_pair_source_create(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item);
void svdf_pair_source_destroy(svdf_pair_source *s);
svdf_dataset *svdf_dataset_from_pair_source(svdf_trainer *t, svdf_pair_source *s, int num_neg, uint64_t seed);
int svdf_pair_source_draw(svdf_trainer *t, svdf_pair_source *s, int num_neg, uint64_t seed, unsigned *neg_out);
int svdf_pair_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, uint64_t seed,
                        unsigned *neg_out);

/* ---- HARD negatives for those passes: the best of num_cand draws by live score.  After a few rounds almost every
 * uniform negative scores far below its positive and its gradient is nearly zero; dynamic negative sampling draws a handful of candidates
 * per positive, scores them with the current model and trains against the best-scoring one.  A hard pass does that in ONE kernel in HBM.
 * THE RULE.  A hard pass has num_neg = m pairs per row and num_cand = C candidates per pair; pair q = r * m + j of row (user_r, pos_r):
 *   candidates  cand(q, i), i = 0 .. C-1, is the negative the rule ABOVE gives pair index q * C + i of a plain pass with m * C negatives per
 *               row and the same seed: cand(q, i) = svdf_pair_negatives(..., num_neg = m * C, seed)[q * C + i].  No new stream, salt or
 *               constant; candidates are outside P(user_r) by construction; repeats among them are allowed; the bound of 4096 draws and the
 *               exhaustion message are the plain pass's, naming the plain-rule pair index q * C + i.
 *   score       score(q, i) = the live-model score of svdf_rank_topn for user user_r and item cand(q, i): i_bias[c] + <W_user[u], W_item[c]>
 *               in float32, every multiply and add rounded separately (no fma): four serial chains a0 .. a3 over the 4-float chunks
 *               (a_t += p[4 j + t] * v[4 j + t]), (a0 + a2) + (a1 + a3), then the up to three tail products added in index order, then
 *               0 + (i_bias + sum).  No user bias, no global bias.  The live model is the model as every call issued earlier on the
 *               trainer's stream leaves it.
 *   selection   neg_q = the candidate with the largest rank key (score, id) among the candidates whose score is not NaN: a higher score
 *               wins; equal scores, +0 == -0, go to the SMALLER item id -- so the result is an id and does not depend on which of two equal
 *               candidates is "first".  +-inf are ordinary scores.  If every candidate scores NaN, neg_q = cand(q, 0).
 *   C = 1 gives the plain pass with num_neg = m, bit for bit.
 * The chosen score (score_out) is score(q, i) of the chosen candidate as computed, -0 kept; where it is a NaN only its being a NaN is
 * specified, not its sign or payload.
 * PINNED VECTORS (seed 12345, num_item 1200, rows (user, pos) = (4, 10), (4, 700), (9, 10)): m = 1, C = 2 has the candidates
 *   pair 0: 607, 549;  pair 1: 766, 1010;  pair 2: 64, 448 -- the six ids pinned above for num_neg 2 -- so with a model whose scores grow
 *   with the item id (W = 0, i_bias[c] = c) the negatives are 607, 1010, 448, and with one whose scores fall with it 549, 766, 64.
 * REFUSED on the host, before any device work and before "needs a GPU", each behind "pair_source: ":
 *   num_neg outside 1 .. 256                  "pair_source: num_neg must be between 1 and 256"
 *   num_cand outside 1 .. 256                 "pair_source: num_cand must be between 1 and 256"
 *   num_neg * num_cand > 256                  "pair_source: num_neg * num_cand must be at most 256"
 *   n * num_neg * num_cand >= 2^31 - 16       "pair_source: n * num_neg * num_cand must stay below 2^31 - 16"
 *   a source of another trainer               "pair_source: the source was created on another trainer"
 *   a trainer svdf_rank_topn does not admit on one GPU (format_type = 1 or extend_type != 0, side tables, common_latent_space, amd:gpus > 1,
 *   a rank handle), in that call's words behind "pair_source: " -- one function admits both.  Every num_factor of the model (1 .. 1024) is
 *   accepted.  svdf_pair_hard_negatives also refuses num_factor outside 1 .. 1024 ("pair_source: hard negatives need num_factor between 1
 *   and 1024").
 * svdf_dataset_from_pair_source_hard returns the data set svdf_dataset_from_pairs builds from (user, pos, neg) of the rule: the same kind,
 * the same schedule or windows, the same trained bits.  Only the step that fills the three columns differs from the plain pass: routes,
 * fallback, refusals and counters 44 / 45 are the plain pass's; counter 46 counts the hard passes among them.  One kernel (k_pair_hard)
 * draws, scores and selects: candidate ids and scores never reach HBM.  Its two forms give the same bits; knob `pair_hard_form` chooses.
 * svdf_pair_source_draw_hard copies the chosen column (and, where score_out is not NULL, the chosen scores) to the host;
 * svdf_pair_hard_negatives is the rule on the host over dense row-major arrays W_user[num_user][num_factor], W_item[num_item][num_factor]
 * and i_bias[num_item] -- no GPU, no handle, the same validation.  No older entry point changes.
 * MEASURED (one MI355X, 100 K users x 10 K items, 20 M shuffled positives, num_neg 1, round against round with the plain pass of the same
 * build, medians of five; profiles/r34_pair_hard.md): num_cand 8 at num_factor 128 adds 32 ms to the 0.280 s round of the exact pass and
 * 36 ms to the 0.179 s round under `amd:step = minibatch`; num_cand 2 adds 13 / 20 ms, num_cand 16 78 / 63 ms.  k_pair_hard takes 29.8 ms
 * there for num_cand 8 (82 GB of item rows from the caches at 2.75 TB/s).  On a planted set, from a cold start, num_cand 8 trained a WORSE
 * ranker than the plain pass; hard rounds after uniform ones were not measured. */
svdf_dataset *svdf_dataset_from_pair_source_hard(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed);
int svdf_pair_source_draw_hard(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed,
                               unsigned *neg_out /* [n*num_neg] */, float *score_out /* [n*num_neg] or NULL: the chosen score */);
int svdf_pair_hard_negatives(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, int num_neg, int num_cand,
                             uint64_t seed, int num_factor, const float *W_user, const float *W_item, const float *i_bias,
                             unsigned *neg_out, float *score_out);

/* ---- ITEM-WEIGHTED negatives for those passes, plain and hard.  Uniform negatives on a skewed catalogue are almost
 * always tail items; the usual remedy draws a negative with probability proportional to an item weight (count^0.75, or any prior of the
 * caller's).  A weighted source is created with item_weight[num_item], uint32, and EVERY pass call above takes it with no new argument.
 * THE RULE, in unsigned integer arithmetic only; G, mix, SALT and stream_q are the plain rule's above, unchanged -- no new stream or constant:
 *   cdf[0]     = 0,  cdf[i + 1] = cdf[i] + item_weight[i],  W = cdf[num_item];  1 <= W <= 2^32 - 1
 *   x(q, t)    = mix(stream_q + (t + 1) * G)                                    ALL 64 bits are used
 *   y          = floor(x * W / 2^64)          the high 64 bits of the 64 x 64 product (__umul64hi; unsigned __int128 on the host)
 *   wdraw(q,t) = the item i with cdf[i] <= y < cdf[i + 1]                       an item of weight 0 is never drawn
 *   neg_q      = the first of wdraw(q, 0), wdraw(q, 1), ... that is not in P(user_r), among the same T = 4096 draws; a pair that exhausts
 *                them fails the call with the plain pass's message.
 * A source whose weights are all equal is NOT the uniform source: the uniform map multiplies the HIGH 32 bits of x by num_item, this one all
 * 64 bits by W.  The two maps agree on all but about num_item of every 2^32 words, so the two sources usually draw the same ids from one
 * seed, but nothing promises it: take the unweighted source where the uniform rule's negatives are wanted.
 * A HARD pass on a weighted source is the hard rule above word for word, cand(q, i) being the WEIGHTED plain rule's negative of pair index
 * q * C + i; score, selection and C = 1 are unchanged.
 * THE DENSITY RULE, WEIGHTED, replaces the count rule for such a source, at creation, in 64-bit integers: a user with rows is refused when
 * 64 * (W - W(P(u))) < W, W(P(u)) the weight of its distinct items (the first such user in id order is named).  Every source that remains
 * accepts each draw with probability >= 1 / 64 less the map's bias of at most W / 2^64 < 2^-32, so the < 1e-28 bound on exhaustion above
 * carries over and no input makes the kernel run long.  The rule bites more often than the count rule: popular items are the ones users hold.
 * PINNED VECTORS (seed 12345, num_item 1200, item_weight[i] = 0 where i % 7 == 0 and 1 + (i * i) % 97 otherwise: W = 50185):
 *   pair 0, draws t = 0 .. 5: 611, 1086, 472, 1016, 936, 514;   pair 7, draws t = 0 .. 7: 502, 551, 33, 918, 200, 19, 1102, 177
 *   rows (user, pos) = (4, 10), (4, 700), (9, 10): num_neg 1 gives the negatives 611, 547, 755; num_neg 2 gives 611, 547, 755, 1006, 59, 447
 *   W = 2^32 - 1 and x = 2^64 - 1 give y = W - 1 = 4294967294.
 * REFUSED on the host, before any device work and before "needs a GPU", after what the plain source refuses about its rows:
 *   a sum of 0                                "pair_source: the item weights sum to 0"
 *   a sum S >= 2^32                           "pair_source: the item weights sum to S: the sum must stay below 2^32"
 *   the density rule                          "pair_source: user U's positive items hold M of the total item weight W: less than 1 part in 64
 *                                              is left to draw a negative from; draw its negatives yourself (svdf_dataset_from_pairs)"
 * svdf_pair_source_create_weighted uploads cdf and a guide table once (two arrays of about num_item and at most 2 * num_item + 1 words); a
 * NULL item_weight is svdf_pair_source_create.  Routes, fallback, refusals and counters 44 / 45 / 46 are untouched; counter 47 counts the
 * passes drawn from a weighted source.  The device reads the map in one of two forms with equal bits (knob `pair_weight_form`): 1 a binary
 * search for y over the whole cdf; 2 a guide table in x space -- Gn the smallest power of two >= max(num_item, 64), guide[g] the item that
 * holds y = mulhi(g << (64 - log2 Gn), W), guide[Gn] the last item of positive weight; a draw reads guide[x >> (64 - log2 Gn)] and its
 * successor and searches cdf between the two, both included.  svdf_pair_negatives_weighted and svdf_pair_hard_negatives_weighted are the
 * rule on the host -- no GPU, no handle, the same validation; a NULL item_weight gives the unweighted calls.
 * MEASURED (one MI355X, 100 K users, 20 M shuffled positives, num_neg 1, medians of five; profiles/r36_pair_weight.md): k_pair_draw on a
 * weighted source takes 1.33 ms (form 2) against 1.36 ms for the uniform source at 10 K items, 1.91 ms (form 1) against 1.70 ms at 100 K
 * items, where form 2 did not pay.  A weighted round (Zipf(0.7) counts to the 0.75, num_factor 128) takes 0.976 s on the exact pass and
 * 0.375 s under `amd:step = minibatch` against 4.31 s / 3.77 s for svdf_pair_negatives_weighted on the host (3.3 s) followed by
 * svdf_dataset_from_pairs -- and against 0.271 s / 0.166 s for the uniform round: negatives that concentrate on popular items make the
 * exact pass's schedule deeper and the windows finer, whoever draws them.  On a planted set weighting did NOT help by the sampled
 * evaluation, whose own negatives are uniform.
 * NOT OFFERED: weighted negatives for the sampled evaluation calls, which draw DISTINCT ids in an open loop; a skewed table needs an
 * admission rule of its own to bound that loop. */
svdf_pair_source *svdf_pair_source_create_weighted(svdf_trainer *t, long n, const unsigned *user, const unsigned *pos_item,
                                                   const unsigned *item_weight /* [num_item], or NULL */);
int svdf_pair_negatives_weighted(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item, const unsigned *item_weight,
                                 int num_neg, uint64_t seed, unsigned *neg_out);
int svdf_pair_hard_negatives_weighted(long num_user, long num_item, long n, const unsigned *user, const unsigned *pos_item,
                                      const unsigned *item_weight, int num_neg, int num_cand, uint64_t seed, int num_factor, const float *W_user,
                                      const float *W_item, const float *i_bias, unsigned *neg_out, float *score_out);

/* ---- SHUFFLED passes: the rows of a source in a fresh order every round, on the device.  SGD on implicit feedback
 * visits its examples in a new order each epoch; the passes above train the rows in the caller's order, the same every round.  A shuffled
 * pass takes one more scalar, order_seed; nothing is permuted on the host, no table is built and nothing is sorted.
 * THE RULE, in unsigned 64-bit arithmetic wrapping mod 2^64; mix and G are the sampled calls' above.  Position p = 0 .. n-1 of the pass holds
 * source row sigma(p), and THE SHUFFLED PASS IS, BIT FOR BIT, THE PASS OF THE SAME KIND (plain, hard, on a weighted source) ON A SOURCE WHOSE
 * ROWS ARE (user[sigma(p)], pos[sigma(p)]), with the same num_neg, num_cand, seed and weights.  P(u), the density rules and the weight table
 * do not depend on the order of the rows; the pair index q = p * num_neg + j counts POSITIONS and the streams are the plain rule's;
 * order_seed and seed are independent (they may be equal).  sigma is a keyed bijection on [0, n): a 4-round unbalanced Feistel network over
 * b bits with cycle walking, O(1) per position:
 *   SALT_ORDER = 0x706169726F726472                  (ASCII "pairordr")
 *   K_i  = mix((order_seed ^ SALT_ORDER) + (i + 1) * G)          i = 0 .. 3
 *   b    = the smallest integer >= 2 with 2^b >= n
 *   E(x): wl = b / 2 (rounded down), wr = b - wl;  L = x >> wr;  R = x & (2^wr - 1)
 *         for i = 0 .. 3:  f = mix(K_i + (R + 1) * G) >> (64 - wl);   (L, R) = (R, L ^ f);   swap(wl, wr)
 *         return (L << wr) | R                                   (after four rounds the widths are the first ones again)
 *   sigma(p): x = p;  repeat x = E(x) until x < n               (at least one application; AT MOST WALKS = 128)
 * Every round maps (L, R) to (R, L ^ f(R)), which is undone by (R', L') -> (L' ^ f(R'), R'): E is a bijection on [0, 2^b), and following E from
 * p until it re-enters [0, n) is one on [0, n).  THE WALK BOUND: for n >= 3, 2^b < 2 n, so a step leaves the range with probability below
 * 1 / 2; if E behaved as a random permutation, some position would need more than 128 steps with probability below n * 2^-128 < 2^-97.  That
 * is a heuristic, not a proof, so the bound is a compile-time constant (as T = 4096 is for the draws): a position that exhausts it fails
 * the call -- on the device through a one-word flag, on the host in the same words -- with
 *   "pair_source: order_seed S needs more than 128 steps at position P; take another order_seed"
 * and no input makes the kernel run long.  WHAT IS PROMISED is the bijection and these bits, NOT a statistically perfect shuffle: four
 * rounds of a hash are not a uniform draw from the n! orders, and at n <= 4 the 24 orders are visibly not equally likely.
 * PINNED VECTORS (order_seed 12345): K_0 .. K_3 = 0x55f0c474c3817246, 0x212e2874c5b74625, 0x1b12a40bba019e32, 0xdbe2e77f7d83df15;
 *   n = 10: sigma = 2, 4, 8, 3, 7, 1, 6, 9, 0, 5;   order_seed 12346, n = 10: 0, 8, 1, 6, 3, 9, 7, 5, 2, 4;
 *   n = 1200, the first eight: 648, 161, 507, 552, 509, 792, 1082, 757;   n = 3: 1, 2, 0;   n = 2: 1, 0;   n = 1: 0 (after four applications)
 *   rows (user, pos) = (4, 10), (4, 700), (9, 10), seed 12345, num_item 1200, num_neg 1: the pass is (4, 700, 607), (9, 10, 549), (4, 10, 766)
 *   -- the negatives pinned above for the plain pass, which belong to positions, on the rows in the order 1, 2, 0.
 * svdf_dataset_from_pair_source_shuffled is svdf_dataset_from_pair_source (num_cand = 0) or svdf_dataset_from_pair_source_hard (num_cand >= 1;
 * num_cand = 1 equals plain) on the permuted rows.  One more kernel (k_pair_order, a lane per position) gathers the rows in the order sigma
 * into two scratch columns of n words, which the draw kernels read in place of the source's; it also counts the adjacent positions that share
 * a user, and ROUTES, FALLBACK, REFUSALS AND COUNTERS 44 .. 47 ARE THE PLAIN PASS'S, DECIDED ON THE PERMUTED ORDER: a shuffled pass over a
 * user-grouped source stays in HBM wherever an ungrouped one does.  Counter 48 counts the shuffled passes among those under 44 / 45.
 * svdf_pair_source_draw_shuffled copies the pass's own three columns (n * num_neg entries each; user_out and pos_out say which row a negative
 * belongs to) and, for num_cand >= 1 with score_out not NULL, the chosen scores.  svdf_pair_order is sigma on the host -- no GPU, no handle;
 * the host rules of a shuffled pass are svdf_pair_negatives* / svdf_pair_hard_negatives* on (user[sigma], pos[sigma]).
 * REFUSED on the host, before any device work and before "needs a GPU": what the plain pass (num_cand = 0) or the hard pass refuses, word
 * for word; svdf_pair_order refuses n < 1 ("pair_source: a source needs at least one row (n >= 1)") and n >= 2^31 - 16 ("pair_source: n *
 * num_neg must stay below 2^31 - 16").  No older entry point changes.
 * MEASURED (one MI355X, 100 K users x 10 K items, 20 M positives, num_factor 128, num_neg 1, medians of five alternating rounds;
 * profiles/r38_pair_order.md): a shuffled round takes 0.272 s on the exact pass and 0.164 s under `amd:step = minibatch`, against 1.33 s /
 * 1.31 s for a host permutation + a new source + a plain pass per round and 3.38 s / 3.28 s for a host permutation + svdf_pair_negatives +
 * svdf_dataset_from_pairs, with bit-equal models; against the unshuffled pass of the same build the order costs 0.4 / 1.6 ms, inside the
 * spreads; k_pair_order takes 0.75 ms.  A user-grouped source takes 14.3 s per unshuffled round (user-run units through the fallback) and
 * 0.281 s per shuffled one -- different passes.  On a planted set a fresh order per round did NOT change the sampled AUC. */
svdf_dataset *svdf_dataset_from_pair_source_shuffled(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed, uint64_t order_seed);
int svdf_pair_source_draw_shuffled(svdf_trainer *t, svdf_pair_source *s, int num_neg, int num_cand, uint64_t seed, uint64_t order_seed,
                                   unsigned *user_out /* [n*num_neg] */, unsigned *pos_out /* [n*num_neg] */, unsigned *neg_out /* [n*num_neg] */,
                                   float *score_out /* [n*num_neg] or NULL: the chosen score of a hard pass */);
int svdf_pair_order(long n, uint64_t order_seed, unsigned *sigma_out /* [n] */);   /* host only: no GPU, no handle */

/* ---- SIMILAR-ITEM lists on the live model: dot and cosine top-N per item.  The calls above answer "which items
 * for this user?"; this one answers "which items are most like this one?" -- related-item shelves, shortlist expansion, a check that the
 * factors mean something -- on the trainer's own model, without an item x item matrix and in the engine's pinned float32 order.
 * Section s of num_section is the QUERY ITEM item[s].  The candidates are all item ids 0 .. num_item - 1; a candidate is RANKED unless it is
 * item[s] itself or is in the section's ban list ban_item[ban_ptr[s] .. ban_ptr[s + 1]) (ban_ptr == NULL: no section has bans).  The query
 * is always excluded; listing it among its own bans is legal; duplicate ban ids count once.
 * THE SCORE of candidate i for query q, by `metric`:
 *   SVDF_ITEM_DOT     0 + (0 + <W_item[q], W_item[i]>), the dot in the pinned order of svdf_rank_topn's score: four serial chains over the
 *                     4-float chunks, each started as 0 + product, then (a0 + a2) + (a1 + a3), then the up to three tail products added in
 *                     index order; every multiply and add rounded separately (no fma).  i_bias is not part of it.
 *   SVDF_ITEM_COSINE  the same expression on the UNIT ROWS R in place of W_item, on both sides: 0 + (0 + <R[q], R[i]>).  For every item i
 *                       ss      = <W_item[i], W_item[i]>   in that same pinned order
 *                       n       = sqrt(ss)                 correctly rounded
 *                       R[i][j] = W_item[i][j] / n         correctly rounded, a DIVISION per element -- not a multiply by a reciprocal,
 *                                                          not rsqrt; denormals are kept, in ss, n and R
 *                     ss == 0 (a zero row, or squares that all underflow) gives R[i] = +0 in every element: such an item scores 0 against
 *                     everything and flags nothing.  Every other input takes the IEEE result of those operations: an overflowing ss gives
 *                     n = inf and elements +-0, or NaN where the element itself is +-inf; a NaN in a row makes its whole unit row NaN, its
 *                     scores NaN, and flags the sections that rank it.  A unit row's self-score is within a few ulp of 1, not 1.
 * OUTPUTS, ORDER AND FLAGS are svdf_rank_topn's word for word: higher score first, equal scores by ASCENDING ITEM ID, +0 == -0;
 *   count_out[s] = min(top_n, num_item - distinct(bans + {item[s]})); item_out / score_out [s * top_n + r] the id and score at rank r, -1 /
 *   0.0f beyond the count; nan_out[s] = 1 empties the list when a ranked candidate scores NaN (a banned NaN row does not flag); score_out
 *   may be NULL; 1 <= top_n <= 256.  Both scores are symmetric in (q, i) bit for bit: the products commute and the order of the sums does
 *   not depend on the side.
 * PINNED VECTORS of the unit rows, bit patterns of the float32 inputs and outputs (tests/test_item_topn.py holds them against the numpy
 * statement of the rule and against svdf_item_unit_rows):
 *   k = 3:  in 3f800000 40000000 c0000000  out 3eaaaaab 3f2aaaab bf2aaaab
 *   k = 5:  in 3dcccccd be4ccccd 3e99999a 3ecccccd bf000000  out 3e0a137d be8a137d 3ecf1d3c 3f0a137d bf2c985c
 *   k = 9:  in 3a83126f 40400000 c0e00000 3f000000 1e3ce508 40200000 be000000 41100000 3e99999a  out 38adcbe3 3e7e95a9 bf1481f8 3d29b91b 1c7a7790 3e542762 bc29b91b 3f3ef03f 3ccbaaee
 *   k = 2:  in 000116c2 80022d85  out 00000000 00000000
 *   k = 3:  in 1a111234 9a911234 1ad99b4d  out 3e81c16b bf01c16b 3f42a220
 *   k = 3:  in 7f61b1e6 bf800000 5f8ac723  out 00000000 80000000 00000000
 * (1, 2, -2; 0.1 .. -0.5; nine mixed magnitudes; two denormals whose squares underflow: the +0 row; three values whose squares are
 * denormal; 3e38, -1, 2e19, whose sum of squares overflows: +-0 elements)
 * REFUSED on the host, before any device work and before "needs a GPU", each behind "item_topn: ":
 *   metric other than 0 / 1                   "item_topn: metric must be 0 (SVDF_ITEM_DOT) or 1 (SVDF_ITEM_COSINE)"
 *   top_n outside 1 .. 256                    "item_topn: top_n must be between 1 and 256"
 *   an id >= num_item in item or ban_item     "sample item index exceed bound" (the ranker's message, as svdf_rank_topn gives it)
 *   ban_ptr not ascending                     "item_topn: ban_ptr must not decrease" ("... must start at >= 0", "ban_item is missing")
 *   NULL outputs with num_section > 0         "item_topn: bad arguments"
 *   a feature_item side table                 "item_topn: a feature_item side table changes an item's effective row ... and is not covered"
 *                                             (a feature_user table does not touch an item row and is admitted)
 *   extend_type 2 / 15, common_latent_space != 0, amd:gpus > 1, a rank handle, a model that is not initialised: svdf_rank_topn_fb's words
 *   behind the new prefix.  format_type = 1 (user-group, SVD++) trainers with extend_type 0 / 1 are ADMITTED: W_item is the same table
 *   there and no feedback list is involved.
 * num_section == 0 returns 0 and launches nothing.  An item may be queried in several sections.  The call runs on the trainer's stream
 * behind whatever is queued and returns when the results are on the host.  The selecting sweeps are svdf_rank_topn's, untouched: they read
 * the sections' query rows (gathered by k_item_query_rows, one launch per piece) in place of W_user rows, for cosine the unit rows (built by
 * k_item_unit_rows, ONE launch per call, never kept across calls -- the model may have moved) in place of W_item, and a zero vector in
 * place of i_bias.  `rank_topn_budget` bounds the list workspace exactly as for svdf_rank_topn; the result does not depend on it.  Counter 49
 * counts the sections listed; counter 39 does not move.
 * svdf_item_unit_rows is the unit-row rule on the host over dense rows[num_row][num_factor] -- no GPU, no handle.
 * MEASURED: profiles/r40_item_topn.md. */
#define SVDF_ITEM_DOT 0
#define SVDF_ITEM_COSINE 1
int svdf_item_topn(svdf_trainer *t, long num_section, const unsigned *item, int metric, const int64_t *ban_ptr, const unsigned *ban_item, int top_n,
                   int *item_out, float *score_out, int *count_out, int *nan_out);
int svdf_item_unit_rows(long num_row, int num_factor, const float *rows, float *out);   /* host function: no GPU, no handle */

/* ---- libc rand() as a random-access stream (the reference draws rank pairs with rand(), apex-tensor/apex_random.h:42-67;
 * SURVEY 8f2).  svdf_rand_peek writes the next n rand() results WITHOUT consuming them, svdf_rand_skip advances the generator
 * by n draws without calling rand() n times (jump-ahead of glibc's additive-feedback table).  Host functions, no GPU needed;
 * the device sampler uses the same machinery.  -1 when libc's generator is not in its default 31-word mode. */
int svdf_rand_peek(long n, int *out);
int svdf_rand_skip(long n);

/* ---- probe of the device-side expf used by the sigmoid links (active_type::map_active / cal_grad call libm's expf,
 * apex_svd_model.h:112-156): out[j] = expf evaluated ON THE GPU for in[j], or, with in == NULL, for the float whose bit
 * pattern is first_bits + j*step_bits.  Tests compare it with the host libm bit for bit.  Needs a GPU. */
int svdf_device_expf(const float *in, unsigned first_bits, unsigned step_bits, float *out, long n);

/* ---- probe of the launch geometry of the live-model ranking calls (DESIGN.md sections 6w, 6x), for tests: what svdf_rank_eval_positions
 * (kind 0) or svdf_rank_topn (kind 1) would launch on this trainer, computed by the very functions those calls use.  Host function, no
 * device work: a host-only handle answers it, before init_model too; only the parameters num_factor and num_item and the knobs
 * rank_eval_budget / rank_topn_budget matter.
 *   kind 0, pos_ptr == NULL: `units` is the number of row tiles of the sweep.
 *   kind 0, pos_ptr != NULL: `units` sections with the positives pos_ptr[0 .. units] and no bans, feedback or lines: the first piece.
 *   kind 1: `units` sections without bans and `top_n`: the first piece.
 * out[0 .. 7] = item ranges (gy), items per range, list capacity (kind 1; else 0), rows of a tile, rows (kind 1: sections) of the piece,
 * its tiles, its sections (0 for kind 0 without pos_ptr), launches of the sweep (the wide evaluation sweep takes one per 32768 rows).
 * A test asserts with it that its shapes reach the geometry it is about.  -1 on bad arguments. */
int svdf_rank_geometry(svdf_trainer *t, int kind, long units, int top_n, const int64_t *pos_ptr, long *out);

/* ---- probe of the launch choice of the level kernels of the exact pass, for tests: what one conflict-free level of n
 * instances would be launched as on this trainer -- by launch_basicmf (launcher 0: one user id, one item id; unit_values: every feature
 * value is 1) or by launch_fused (launcher 1: at most max_nu and max_ni ids, each 1 or 2; has_globals: the data set has global features) --,
 * computed by the very functions those launchers use.  Host function, no device work: a host-only handle answers it, before init_model too;
 * only the parameters and the knobs matter.  out[0 .. 19] =
 *    0 form: 1 k_basicmf FULL / FAST, 2 k_basicmf general stream with unit values, 3 k_basicmf with feature values, 4 k_basicmf_slots eight lanes
 *      (k = 64), 5 k_basicmf_slots sixteen lanes (k = 256), 6 k_fused, 7 k_fused hot-reduce, 8 k_fewrow_fast, 9 k_fewrow_slots sixteen lanes (k = 128)
 *    1 lane class of the width, 2 lanes per row, 3 chunks per lane, 4 full rows (no per-lane bounds test), 5 row sets per wave after folding,
 *    6 threads per workgroup, 7 / 8 user / item slots of the few-row template, 9 instances per row set, 10 instances per workgroup,
 *    11 workgroups with work, 12 workgroups launched, 13 XCD remap on, 14 row gathers (0 plain, 1 nontemporal), 15 row stores (0, 1, 2),
 *    16 the knobs the launch reads (1 groups_per_wave, 2 block_threads, 4 xcd_remap, 8 load_mode, 16 store_mode),
 *    17 dynamic LDS bytes, 18 the configuration has a chained form, 19 the widest level handed to it (0: none; chain_width)
 * -1 on bad arguments. */
int svdf_level_geometry(svdf_trainer *t, int launcher, long n, int max_nu, int max_ni, int unit_values, int has_globals, long *out);

/* ---- probe of the map of a weighted pair source, for tests: id_out[j] = the item the rule above gives the 64-bit
 * word x[j] under item_weight[num_item], by the very function the draw kernels call.  form 1 or 2 as knob pair_weight_form (0: the knob's
 * choice).  t == NULL: on the host, no GPU.  With a trainer: the tables are uploaded and the function runs on the device in one small launch
 * (a host-only handle answers "needs a GPU").  The weights are validated as a weighted source validates them.  -1 on bad arguments. */
int svdf_pair_weight_lookup(svdf_trainer *t, long num_item, const unsigned *item_weight, int form, long nx, const uint64_t *x, unsigned *id_out);

/* ---- probes of the window rule of `amd:step = minibatch` (svdf_wseq_rule.h): into how many windows a pass is cut, from knob values and
 * counts alone.  Host functions, no handle and no GPU; the data-set builders reach the same functions.  Tests compare them with
 * tests/window_rule.py.
 * svdf_window_rule: the per-pass rule of one route -- 0 instances given as columns (ratings, rank pairs; item_count, the item lane),
 * 1 rows (svdf_dataset_from_csr: all three counts, the child marks, both lanes), 2 user-group blocks (the counts, fb_mass, num_block, both
 * lanes).  Returns the window count, -1 on an unknown route.  A lane with sub == 0 is off; a mark array may be NULL (no side table). */
typedef struct svdf_window_rule_in {
    int per_target, per_target_max, per_target_fb, per_target_shared, per_target_child; /* the knobs window_per_target ... */
    long window;                              /* amd:window rows, 0 = unset */
    int shared_sub, shared_cap, item_sub, item_cap; /* the lanes of ordered sub-steps: window_shared_sub / _max and their kin */
    long n, num_block;                        /* instances of the pass; blocks (route 2) */
    long num_item, num_global, num_shared;    /* lengths of the count (and mark) arrays */
    const int64_t *item_count, *global_count, *shared_count; /* updates per pass of every item row, global bias, shared user row */
    const unsigned char *item_child, *shared_child; /* rows that are a feature_item / feature_user child somewhere */
    long num_fb;
    const double *fb_mass;                    /* per feedback row: instance-sized updates per pass (route 2) */
} svdf_window_rule_in;
long svdf_window_rule(int route, const svdf_window_rule_in *in);
/* the rule on the windows as cut, one class of rows over `ncol` id columns of n rows each (ids < num_id): from W, more windows at equal
 * positions until the mean over entries of min(count of the entry's row in its window, sub) (sub 0: the count) is within target * slack
 * and the most updates of one row in one window within cap * slack; after `rounds` scans, or past n windows, n.  -1 on bad arguments. */
long svdf_window_rule_as_cut(long W, long n, int ncol, const unsigned *const *cols, long num_id, double target, long cap, int sub,
                             double slack, int rounds);
/* the cut of num_block user-group blocks into W windows: W + 1 block positions into cut_out, even positions moved forward to where no
 * START .. END span is open.  -1 on bad arguments. */
int svdf_window_block_cuts(long num_block, const int *extend_tag, long W, long *cut_out);

/* ---- host-side conflict-free batch scheduler, exposed so it can be tested without a GPU.
 * Unit r touches resources res[res_ptr[r] .. res_ptr[r+1]) out of num_res.  Writes the batch-sorted
 * (stable) unit order and level_ptr[0..nlevels]; returns the number of batches, -2 if level_cap
 * (capacity of level_ptr_out) is too small. */
int svdf_schedule_resources(long n, const int64_t *res_ptr, const unsigned *res, long num_res, int *order_out,
                            int64_t *level_ptr_out, long level_cap);

#ifdef __cplusplus
}
#endif
#endif /* SVDFEATURE_AMD_H_ */

// svdf_engine.h -- host side of the MI355X apex_svd engine (one instance == one ISVDTrainer).
//
// Mirrors the call protocol of the reference's base solver (solvers/base-solver/apex_svd_base.h)
// behind the C ABI of include/svdfeature_amd.h.  The host does: config parsing, model file I/O,
// rand_init (libc rand(), bit-identical start), staging of borrowed instances, and the
// CONFLICT-FREE BATCH SCHEDULER that turns the reference's strictly sequential SGD into
// dependency-respecting parallel launches.  All arithmetic on parameters
// happens in the HIP kernels (svdf_k_*.hip); there is no CPU compute fallback.
#ifndef SVDF_ENGINE_H_
#define SVDF_ENGINE_H_

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <string>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <vector>

#include "svdf_types.h"

namespace svdf {

struct Error : std::runtime_error {
    explicit Error(const std::string &m) : std::runtime_error(m) {}
};
[[noreturn]] void fail(const std::string &msg);
// true while the calling thread runs the multi-GPU code of an amd:gpus handle (svdf_engine.cpp)
bool in_multi_scope();
void pin_malloc_threshold();   // svdf_engine.cpp: glibc's dynamic mmap threshold off, once per process, from the ranker only (see there)
struct MultiScope { MultiScope(); ~MultiScope(); MultiScope(const MultiScope &) = delete; MultiScope &operator=(const MultiScope &) = delete; };

// --------------------------------------------------------------------------- device memory
// A handle's cache of device blocks (svdf_staged.cpp): while a DevPoolScope is open on the calling thread, DevBuf takes its blocks from the
// pool and gives them back to it instead of hipMalloc / hipFree (a hipFree waits for the device).  The transient window sequences of the
// staged route are built, trained once and dropped every stage_window rows inside such a scope: their blocks go round.
// The pool holds a WHOLE sequence, however many windows it has (blocks ordered by size; no cap on their number).  It is trimmed at the end
// of every chunk: a block that no buffer took during the last two chunks is freed, so the pool follows the size of the recent sequences.
// A hipMalloc that fails inside a scope empties the pool and is tried once more.
// Everything that reads or writes a block is ordered on the handle's ONE stream, so a block may change hands while kernels are still queued.
struct DevPool {
    struct Block { void *p; long gen; };
    std::multimap<size_t, Block> blocks;     // by size in bytes
    long gen = 0;                            // chunks finished so far (end_chunk)
    int64_t n_taken = 0, n_missed = 0;       // requests served from the pool / by hipMalloc inside a scope
    DevPool() = default;
    DevPool(const DevPool &) = delete;
    DevPool &operator=(const DevPool &) = delete;
    ~DevPool() { drop(); }
    void drop();
    void *take(size_t bytes, size_t &got);   // nullptr: nothing that fits
    void give(void *p, size_t bytes);
    void end_chunk();                        // trims what the last two chunks did not use
};
DevPool *dev_pool_current();                 // the pool of the calling thread's open scope, or nullptr
struct DevPoolScope {
    DevPool *prev;
    explicit DevPoolScope(DevPool *p);
    ~DevPoolScope();
    DevPoolScope(const DevPoolScope &) = delete;
    DevPoolScope &operator=(const DevPoolScope &) = delete;
};
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) {
            if (DevPool *pool = dev_pool_current()) pool->give(p, cap * sizeof(T));
            else (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
    }
    void reserve(size_t n) {           // grow-only, contents not preserved
        const hipError_t e = try_reserve(n);
        if (e != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e) + " at hipMalloc (DevBuf::reserve)");
    }
    hipError_t try_reserve(size_t n) { // reserve() that hands the allocation's error to a caller with more to say about it
        if (n <= cap && p) return hipSuccess;
        release();
        const size_t want = n ? n : 1;
        DevPool *pool = dev_pool_current();
        if (pool) {
            size_t got = 0;
            if (void *q = pool->take(want * sizeof(T), got)) { p = static_cast<T *>(q); cap = got / sizeof(T); return hipSuccess; }
        }
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess && pool && !pool->blocks.empty()) {   // the cached blocks may be what is in the way
            (void)hipGetLastError();
            pool->drop();
            e = hipMalloc((void **)&p, want * sizeof(T));
        }
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void upload(const T *src, size_t n, hipStream_t st) {
        reserve(n);
        if (!n) return;
        hipError_t e = hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) fail(std::string("HIP error: ") + hipGetErrorString(e) + " at hipMemcpyAsync (DevBuf::upload)");
    }
};

// --------------------------------------------------------------------------- scheduler (pure host)
// Assigns every unit (instance or SVD++ user) the earliest batch in which none of its parameter
// rows is touched by an earlier unit of the same or a later batch:
//   level(t) = 1 + max(last[r] for r in resources(t)),  last[r] = level(t)
// Units of one level share no resource, units that share a resource keep their file order, so
// executing levels in increasing order reproduces the sequential result exactly.
struct LevelTracker {
    std::vector<int> last;   // per resource: level of the most recent unit touching it
    int base = 0;            // levels <= base belong to work already enqueued
    void resize(size_t nres) { if (last.size() < nres) last.resize(nres, 0); }
};
struct Schedule {
    std::vector<int> order;        // unit ids sorted by level, stable
    std::vector<long> level_ptr;   // level l occupies order[level_ptr[l] .. level_ptr[l+1])
    std::vector<long> level_mid;   // user-unit schedules only: [level_ptr[l], level_mid[l]) are the fast-path (UNIT_SIMPLE) units
    long max_level_size = 0;
    size_t num_levels() const { return level_ptr.empty() ? 0 : level_ptr.size() - 1; }
};
// levels[t] must already hold each unit's level (> tracker.base); builds order/level_ptr.
void build_schedule(const std::vector<int> &levels, int base, Schedule &out);

struct SideTable {   // SparseFeatureArray<float> (apex-utils/apex_utils.h:140-196)
    std::vector<unsigned> row_ptr{0};
    std::vector<unsigned> index;
    std::vector<float> value;
    unsigned num_row() const { return (unsigned)row_ptr.size() - 1; }
    void load(const char *fname);
};
struct ParamSet {    // ParameterSet (apex_svd_base.h:33-75)
    std::vector<float> wd;
    std::vector<unsigned> bound;
    std::string prefix_a, prefix_b;
    void set_param(const char *name, const char *val);
};

struct HostCSR {     // staged SVDFeatureCSR rows (apex_svd_data.h:109-127)
    std::vector<float> row_label;
    std::vector<int> row_ptr{0};
    std::vector<unsigned> feat_index;
    std::vector<float> feat_value;
    long num_row() const { return (long)row_label.size(); }
    void clear() { row_label.clear(); row_ptr.assign(1, 0); feat_index.clear(); feat_value.clear(); }
};

// level-sorted SoA form of few-row instances (FusedSchedule) on the host and in HBM
struct FusedHost {
    std::vector<float> label, uval[2], ival[2], gval;
    std::vector<unsigned> uidx[2], iidx[2], gidx;
    std::vector<int> gptr;
    std::vector<unsigned> gsi[4];   // inline global slots, filled when every instance has <= 4 distinct global ids
    std::vector<float> gsv[4];
    int max_nu = 1, max_ni = 1;
    bool has_g = false, inline_g = false;
};
struct FusedDev {
    DevBuf<float> label, uval[2], ival[2], gval, gsv[4];
    DevBuf<unsigned> uidx[2], iidx[2], gidx, gsi[4];
    DevBuf<int> gptr;
    int max_nu = 1, max_ni = 1;
    bool has_g = false, inline_g = false;
    bool dense_slots = false;   // every instance has exactly one user id and one item id (k_fewrow_gslots reads slot 0 without an absent test)
    void upload(const FusedHost &h, hipStream_t st);
    FusedSchedule view() const;
};

// user-group (SVD++) stream in HBM: CSR rows + feedback lists + unit records + batch order
struct UnitDev {
    DevBuf<float> label, value, fbval;
    DevBuf<int> ptr, order;
    DevBuf<unsigned> index, fbidx;
    DevBuf<DevUnit> units;
    DevBuf<DevUnitX> xunits;       // the same units in launch order with their first row entry and user id (k_svdpp_wave)
    DevBuf<DevBlk> blks;           // extend_type 2: the blocks the units range over
    DevBuf<unsigned char> fresh;   // DevCSR::row_fresh (allocated only when some row needs it)
    bool has_fresh = false, unit_values = false;
    DevCSR csr() const { return DevCSR{label.p, ptr.p, index.p, value.p, unit_values ? 1 : 0, has_fresh ? fresh.p : nullptr}; }
};

// One instance of a user block as PairwiseRankGenerator sees it (SVDFeatureCSR::Elem, apex_svd_data.h:38-107): the
// global, user and item entries are contiguous in that order.
struct RankRow {
    float label;
    int ng, nu, ni;
    const unsigned *index;
    const float *value;
};

// libc rand() as a random-access stream (svdf_randstream.cpp): the generator's last 31 values, oldest first
struct WUnitHost;   // one window's host-built arrays of the user-unit step (svdf_internal.h)
struct WseqCounts;  // updates per shared target of a pass, for the window rule (svdf_wseq_rule.h)
struct WseqKnobs;   // the knob values the window rule reads (svdf_wseq_rule.h)
struct WseqLane;    // a lane of ordered sub-steps: its sub-step and its cap (svdf_wseq_rule.h)
struct LibcRand { uint32_t x[31]; char *handle = nullptr; };
bool libc_rand_capture(LibcRand &s);
void libc_rand_restore(const LibcRand &s);
void libc_jump_poly(uint64_t J, uint32_t a[31]);
void libc_rand_chunk_states(const LibcRand &s0, long nchunks, long C, std::vector<uint32_t> &states);
void libc_rand_peek(long n, int *out);
void libc_rand_skip(long n);

// PairwiseRankGenerator (apex_svd_data.cpp:812-1025) restated for whole passes: the rows of a user block are replaced by
// rank pairs drawn with libc rand() in the reference's call order, so that a seeded run sees the same pairs.
class PairSampler {
public:
    void set_param(const char *name, const char *val);   // apex_svd_data.cpp:971-981
    void init();                                          // apex_svd_data.cpp:982-988 (once per handle)
    // appends the rows generated from one block; row_ptr holds absolute value offsets and starts as {0}
    void sample_block(const std::vector<RankRow> &rows, std::vector<float> &label, std::vector<int64_t> &row_ptr,
                      std::vector<unsigned> &index, std::vector<float> &value);
    // what the device sampler (svdf_k_sample.hip) needs to know
    int method() const { return method_; }
    int pointwise() const { return pointwise_; }
    int sample_num() const { return sample_num_; }
    int sample_max() const { return sample_max_; }
    float pos_lowerb() const { return pos_lowerb_; }
    float neg_upperb() const { return neg_upperb_; }
    int seed_bytime() const { return seed_bytime_; }
    float gap() const { return gap_; }
private:
    int sample_num_ = -1, sample_max_ = 0x7fffffff, method_ = 0, pointwise_ = 0, seed_bytime_ = 0;
    float gap_ = 0.0001f, pos_lowerb_ = 0.8f, neg_upperb_ = 1e-6f;
    bool init_done_ = false;
    std::vector<RankRow> pos_, neg_;
};

struct RankPrefetch;
struct UserGroupArrays;
struct MultiState;                                   // svdf_multi.cpp: the other ranks of an "amd:gpus = N" handle
struct MultiDeleter { void operator()(MultiState *m) const; };
struct IpcState;                                     // svdf_ipc.cpp: IPC-mapped wire buffers / flag pages of the one-process-per-GPU ranks
struct IpcDeleter { void operator()(IpcState *s) const; };
struct RcclState;                                    // svdf_rccl.cpp: the rank's own RCCL communicator, side stream and hand-over buffers
struct RcclDeleter { void operator()(RcclState *s) const; };
void rccl_unique_id(unsigned char *out128);
// a user-group buffer file kept in HBM for the device sampler (svdf_k_sample.hip); built once per file, reused every pass
struct RankSource {
    std::string path;
    long file_size = -1, file_mtime = -1, file_ino = -1;   // cache key: size, mtime in ns, inode
    bool eligible = false;
    bool unit_values = false;   // eligible and every row's user and item value is exactly 1 (pair windows carry unit values)
    long num_block = 0, num_row = 0;
    DevBuf<long> block_row_ptr, draws, pairs, draw_off, pair_off;
    DevBuf<float> label, uval, ival;
    DevBuf<unsigned> uidx, iidx, raw, tables;
    DevBuf<int> pos_list, neg_list;
    // the general device sampler (svdf_k_gsample.hip): the file's rows in the reference's CSR layout, the host copy of everything a
    // generated pass keeps from the file (tags, feedback lists), and the pass's scratch / output
    bool general = false;
    std::vector<int> h_tag;
    std::vector<int64_t> h_fb_ptr;
    std::vector<unsigned> h_fb_index;
    std::vector<float> h_fb_value;
    DevBuf<int> g_row_ptr, pair_p, pair_n, lens, optr;
    DevBuf<unsigned> g_index, out_index;
    DevBuf<float> g_value, out_label, out_value;
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    ~RankSource() { if (scan_tmp) (void)hipFree(scan_tmp); }
};
class Engine;
class Ranker;

// HBM-resident scheduled training set
struct Dataset {
    Engine *owner = nullptr;
    long num_row = 0;
    int kind = 0;                 // 0 basicMF fused kernel, 1 general sparse kernel, 2 few-row fused kernel, 3 SVD++ units, 4 multi-level units, 9 ratings with hot rows (svdf_pivot.cpp),
                                  // 5 window-minibatch (user-grouped instances of one exchange window, svdf_k_window.hip)
    // kind 5: user records in launch order, user-grouped columns (item / label / uval / ival above), contribution slots, item segments
    DevBuf<WinUser> win_urec;
    DevBuf<int> win_slot, win_iptr, win_slot1;
    DevBuf<unsigned> win_item1;   // rank pairs: the second (higher-id) item entry, its slot and sign; entry 0 uses item / win_slot / ival
    DevBuf<float> win_ival1;
    long win_item_lo = 0, win_item_hi = -1;   // kind 5: lowest / highest item id with an instance in the window (-1: none)
    DevBuf<long> d_level_ptr;     // kind 2: the level boundaries in HBM, uploaded when a run of narrow levels is first chained (k_fewrow_slots_chain)
    bool d_level_ptr_ok = false;
    // kind 10: runs of an item's consecutive ratings (svdf_runs.cpp): level-sorted columns of the runs; user / item / label above stay in FILE order
    // kind 11: user-run units of rank pairs (svdf_punit.cpp): pu_units in launch order (sched.level_ptr over units), pair columns in file order
    DevBuf<PairUnit> pu_units;
    DevBuf<unsigned> pu_lo, pu_hi;
    DevBuf<float> pu_vlo, pu_one;
    DevBuf<unsigned> rn_item, rn_user[8];
    DevBuf<float> rn_label[8];
    int rn_len = 0;
    // ... their order inside a level (knob "runs_order" when the data set was built): 1 = longest runs first, item order inside a length, 0 = item order.
    // Counted in HBM once per data set over the aligned row sets a wave of the pass kernel carries (svdf_dataset_info 11 / 12): the sum of every set's
    // longest run = the steps the waves walk, the sets whose runs differ in length; rn_hist[length] = runs of that length
    int rn_order = 0;
    int64_t rn_wave_steps = 0, rn_mixed_sets = 0, rn_hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // ... and their operand staging (knob "runs_stage"; svdf_runs.cpp: runs_stage_build): slot s * (1 + rn_len) + j, run-major, indexes rn_dst and rn_stage_bias; the
    // slot's row is row j * num_units + s of rn_stage_row; rn_first[r] = the slot of row r's first touch; rn_label_rm[s * rn_len + j] = rn_label[j][s]
    DevBuf<float> rn_stage_row, rn_stage_bias, rn_label_rm;
    DevBuf<unsigned> rn_dst, rn_first;
    int rn_stage_state = 0;       // 0 not tried yet, 1 built, 2 refused (the gate, or no memory): the data set keeps reading and writing W
    unsigned rn_stage_row0 = 0;   // the W row of user 0 the HOME words were built against
    int64_t rn_stage_bytes = 0;
    // kind 9: hot rows walked as units (svdf_pivot.cpp): sched.level_ptr = the cold ratings' level boundaries (user / item / label above),
    // pv_unit_ptr = the units' (unitdev.xunits in launch order, their rows in unitdev)
    std::vector<long> pv_unit_ptr;
    bool pv_item_pivot = false;
    long pv_cold = 0, pv_hot_rows = 0;
    int64_t chained_levels = 0;   // levels the current launch sequence of this data set walks inside chained launches
    bool win_hot = false;         // kind 5 inside a one-GPU sequence: some item has more than window_hot_sub (rank pairs: window_pair_sub) slots in this window (ordered sub-steps: k_window_apply / k_window_apply_pairs)
    long win_slots = 0;           // contribution slots of the window = item entries (kind 7: + feedback entries)
    // kinds 5 and 7 of a resident data set (a one-GPU sequence's child, a stand-alone svdf_dataset_window_from_*): row r of the regrouped columns
    // was row win_pos[r] of the window's source range -- what svdf_predict_dataset reports file order through.  Windows of
    // staged chunks and of amd:gpus shards are built without it.
    DevBuf<int> win_pos;
    bool win_has_pos = false;
    std::vector<long> wfirst;     // kind 8: the first file row of every child (children cover consecutive file ranges)
    // kind 7: window-minibatch data set of user units (svdf_k_wunit.hip): user-group blocks / rows with global features
    DevBuf<WinUnit> wu_units;
    DevBuf<WinSeg> wu_segs;
    DevBuf<int> wu_rptr, wu_tptr, wu_gptr;
    DevBuf<WinEnt> wu_ent, wu_fbent;
    DevBuf<WinTouched> wu_touched; // one-GPU window sequences: targets with slots (in-place sums)
    long wu_ntouched = -1;         // -1: no list
    DevBuf<WinFbRec> wu_fbrec;    // deferred feedback scatter: slot-ordered (segment, value) records; empty = the walk writes contribution rows
    long wu_nseg = 0;
    bool wu_defer_fb = false;
    long wu_gslots = 0;           // contribution words of the global biases = global entries
    int wu_estride = 0;           // > 0: every row has wu_estride - 1 global entries and one item entry (no row pointer array)
    bool wu_feedback = false;     // the units carry implicit-feedback lists (user-group trainer)
    DevBuf<int> wu_uptr, wu_upos;  // shared user entries (amd:shared_user_from): per-row ranges into wu_uent and the private entry's position
    DevBuf<WinEnt> wu_uent;
    long wu_nshared = 0;           // > 0: the window has shared user entries; targets [.., + wu_nshared) are user rows B .. num_user - 1
    bool wu_shared_uniform = false;   // user-group windows: every segment's rows carry one user section of at most 4 shared entries (the wave walk's form)
    DevBuf<int> wu_iptr;           // feature_item children of the window's item entries: per-row ranges into wu_ient
    DevBuf<WinEnt> wu_ient;
    bool wu_ichild = false;        // the window has feature_item children
    DevBuf<WinHot> wu_hot;         // hot shared user rows of the window (ordered sub-steps, knob window_shared_sub) and their records
    DevBuf<WinHotRec> wu_hrec;
    long wu_nhot = 0;              // hot shared user rows: wu_hot[0 .. wu_nhot)
    long wu_nihot = 0;             // hot item rows (knob window_item_sub): wu_hot[wu_nhot .. wu_nhot + wu_nihot), records in wu_hrec too
    int wseq_shared_sub = -1;      // kind 8 from wseq_from_csr (else -1): window_shared_sub when the sequence was built (train_dataset refuses another value)
    int wseq_item_sub = -1;        // the same for window_item_sub
    int wseq_block_sub = -1;       // kind 8 from wseq_from_blocks (else -1): window_block_sub as it took effect when the sequence was built (0 without amd:shared_user_from; train_dataset refuses another value)
    int wseq_block_item_sub = -1;  // the same for window_block_item_sub (hot item rows of SVD++ blocks; 0 on trainers that are not user-group)
    long wu_nhrec = 0;             // records in wu_hrec (user-group windows: the rows of the trainer's second record plane, d_hfb_ / d_hfbb_)
    bool plain_rows = false;       // built by dataset_from_triples / _from_pairs through the general representation (side tables, wide rows ...): the default-step guard names the window step by the columns' shape
    int wseq_hot_sub = -1;         // kind 8 from wseq_from_triples (else -1): window_hot_sub as it took effect when the sequence was built (0 without the lane; train_dataset refuses another value)
    int wseq_pair_sub = -1;        // kind 8 from wseq_from_pairs (else -1): window_pair_sub when the sequence was built (train_dataset refuses another value)
    // kind 8: one GPU, `amd:step = minibatch`: the pass as a sequence of windows (kind 5 or kind 7 children), each trained and applied in place
    std::vector<Dataset *> wchild;
    // kind 6: a data set of an amd:gpus = N handle (svdf_multi.cpp): mchild[rank][window] lives in that rank's HBM
    std::vector<std::vector<Dataset *>> mchild;
    bool m_minibatch = false;     // the children are window-minibatch data sets (kind 5), else level-scheduled ones
    FusedDev fused;               // kind 2
    UnitDev unitdev;              // kind 3: user-group (SVD++) units
    Schedule sched;               // level_ptr always; order on the host only when built there or asked for (host_order)
    DevBuf<int> order_dev;        // device-built schedules: the unit order stays in HBM until a prediction needs it un-permuted
    // kind 0: level-sorted compact records
    DevBuf<unsigned> user, item;
    DevBuf<float> label, uval, ival;
    bool unit_values = true;
    // kind 1: CSR stream + order
    DevBuf<float> row_label, feat_value;
    DevBuf<int> row_ptr, order;
    DevBuf<unsigned> feat_index;
    long algorithmic_bytes = 0;
    long num_units = 0, num_simple_units = 0;
    uint64_t sched_signature = 0;  // Engine::schedule_signature() at build time
    // captured launch sequence of one pass (Engine::train_dataset)
    hipGraphExec_t graph_exec = nullptr;
    uint64_t graph_version = 0;
    hipStream_t graph_stream = nullptr;
    Dataset() = default;
    ~Dataset();
    Dataset(const Dataset &) = delete;
    Dataset &operator=(const Dataset &) = delete;
};

// A resident source of positives (user, item) for passes of rank pairs whose negatives the device draws (svdf_pairsource.cpp; DESIGN.md
// section 6ac): one upload each at creation, nothing per pass.  A host-only handle's source holds no device memory.
struct PairSource {
    Engine *owner = nullptr;
    long n = 0;
    long same = 0;                     // rows whose user is the row's before: the user-column pretest of user-run units, from the caller's column
    DevBuf<unsigned> user, pos, uitems;   // [n], [n], every user's distinct items ascending
    DevBuf<int> uptr;                  // [num_user + 1]
    bool weighted = false;             // created with item weights (section 6ae): negatives are drawn through the tables below
    DevBuf<unsigned> cdf, guide;       // [num_item + 1], [Gn + 1] (svdf_pairweight_lists.h)
    unsigned weight_sum = 0;           // W
    int weight_shift = 0;              // 64 - log2 Gn
    PairSource() = default;
    ~PairSource();
    PairSource(const PairSource &) = delete;
    PairSource &operator=(const PairSource &) = delete;
};

struct RankLines;   // the USER lines of the svdf_rank_*_lines calls (svdf_ranklines_lists.h)
struct RankTopnLists;   // the validated ban lists of the top-N calls (svdf_ranktopn_lists.h)
class Engine {
  public:
    Engine(TypeParam mtype, int device);
    ~Engine();

    // ISVDTrainer surface
    void set_param(const char *name, const char *val);
    void init_model();
    void load_model(FILE *fi);
    void save_model(FILE *fo);
    void save_model_begin(FILE *fo);   // the file written beside the next pass (svdf_model.cpp)
    void save_model_end();
    void init_trainer();
    void set_round(int nround);
    void finish_round();
    void update_csr(float label, int ng, int nu, int ni, const unsigned *index, const float *value);
    float predict_csr(float label, int ng, int nu, int ni, const unsigned *index, const float *value);
    void update_csr_batch(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value);
    void predict_csr_batch(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value, float *out);
    void update_block(int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row, const float *row_label,
                      const int *row_ptr, const unsigned *feat_index, const float *feat_value);
    void predict_block(int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row, const float *row_label,
                       const int *row_ptr, const unsigned *feat_index, const float *feat_value, float *out);

    // resident datasets
    Dataset *dataset_from_csr(long num_row, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    Dataset *dataset_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    Dataset *dataset_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg);
    Dataset *dataset_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                 const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                 const float *feat_value);
    // the reference's binary buffer files, read natively (svdf_buffer.cpp): CSR buffer or user-group buffer
    Dataset *dataset_from_buffer_file(const char *path, int user_group_format);
    // input_type = 2: a user-group buffer file through the rank-pair sampler, one pass per call
    Dataset *dataset_from_rank_buffer_file(const char *path);
    long rank_sample_buffer_file(const char *in_path, const char *out_path);   // host only; returns the number of rows written
    // draws the NEXT pass on a background thread; the next dataset_from_rank_buffer_file / rank_sample_buffer_file call
    // for the same file takes it.  Nothing else may call rand() until then (the reference's loop does not, svd_feature.cpp:272-283)
    void rank_prefetch(const char *path);
    void rank_prefetch_drop();
    // window-minibatch data set of one exchange window (N > 1 ranks: user side exact, item side one minibatch step per window)
    Dataset *dataset_window_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    Dataset *dataset_window_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg);
    void window_delta_pack(Dataset *ds, void *device_dst, int half, int64_t *count);   // per-item sum of the window's contributions -> wire buffer
    void window_delta_apply(const void *device_src, int half);                           // replicated ranges += wire buffer
    void window_delta_apply_local(Dataset *ds);                 // stratified schedule: the active item block += the window's per-item sums, in place
    // cross-process direct exchange through IPC-mapped buffers (svdf_ipc.cpp)
    void ipc_setup(int rank, int world, int64_t wire_bytes, int64_t block_floats, unsigned char *handles_out);
    void ipc_connect(const unsigned char *all_handles);
    void ipc_window_pack(Dataset *ds, int half);
    void ipc_window_reduce(int half);
    void ipc_window_apply(int half);
    void ipc_block_send(int dst, int slot);
    void ipc_block_recv(int src, int slot, unsigned seq);
    int ipc_status() const;
    void ipc_set_spin_limit(long polls);       // knob "ipc_spin_limit": polls before a flag wait gives up (tests; default ~ several seconds)
    long ipc_spin_limit_ = 0;
    void ipc_fail_if_dead(const char *where);   // raised by svdf_synchronize: a timeout in the last window must not pass silently
    void ipc_close();
    // the same exchanges issued from C++ straight into RCCL (svdf_rccl.cpp)
    void stratum_step(Dataset *const *ds, int n, int block, int nblocks, float *device_out);
    void item_block_set_at(int block, int nblocks, const float *device_src);
    void rccl_init(const unsigned char *id128, int rank, int world);
    void rccl_window_allreduce(Dataset *ds, int half);
    void rccl_block_handoff(int dst, int src, int slot, int in_block, int nblocks);
    void rccl_block_arrive(int slot);
    int64_t rccl_counter(int what) const;
    void rccl_close();
    // the same step for user units (svdf_k_wunit.hip): rows with global features / several item entries, user-group (SVD++) blocks
    Dataset *dataset_window_from_csr(long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    Dataset *dataset_window_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                        const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                        const float *feat_value);
    void item_block_copy(float *device_buf, int set, int64_t *count);   // the active partition of the replicated ranges <-> a packed fp32 buffer
    void train_dataset(Dataset *ds);
    void predict_dataset(Dataset *ds, float *out);
    void eval_dataset(Dataset *ds, float scale, double *sum_sq, int64_t *count);
    // batch ranking evaluation on the live model (svdf_rankeval.cpp, svdf_k_rankeval.hip)
    void rank_eval_positions(long S, const unsigned *user, const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr,
                             const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out, int *nan_out);
    // top-N item lists on the live model (svdf_ranktopn.cpp, svdf_k_ranktopn.hip)
    void rank_topn(long S, const unsigned *user, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out, float *score_out,
                   int *count_out, int *nan_out);
    void rank_live_refusals(const char *who, bool svdpp_ok = false, bool tables_ok = false);   // the configurations the batch ranking calls do not cover
    // the same calls for sections with feedback lists: user-group (SVD++) trainers (svdf_k_rankrows.hip)
    void rank_eval_positions_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out,
                                int *nan_out);
    void rank_topn_fb(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                      const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out);
    bool rank_live_fb_refusals(const char *who, bool has_lists, bool tables_ok = false);
    // the same calls for sections that bring a USER line (several ids, any value) and for trainers with feature_user / feature_item side
    // tables (svdf_k_rankrows.hip)
    void rank_eval_positions_lines(long S, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                                   const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out,
                                   int *ranked_out, int *nan_out);
    void rank_topn_lines(long S, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                         const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out);
    void rank_lines_admit(const char *who, long S, const RankLines &U);   // the lines and the tables' child ids, on the host
    void rank_live_items(const char *who, const float **item_rows, const float **item_bias);   // the prepared item side where feature_item is set
    // lines != nullptr: a _lines call -- `user` is not read, the rows come from the lines (and fb_ptr, where the trainer is a user-group one)
    void rank_eval_run(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *pos_ptr,
                       const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int *position_out, int *tied_out, int *ranked_out,
                       int *nan_out, const RankLines *lines = nullptr);
    void rank_geometry(int kind, long units, int top_n, const int64_t *pos_ptr, long *out);   // test probe (svdf_rank_geometry): host only
    void level_geometry(int launcher, long n, int max_nu, int max_ni, int unit_values, int has_globals, long *out);   // test probe (svdf_level_geometry): host only
    void level_config(DevParams &P, int pitch) const;   // the DevParams fields the launch choice of the level kernels reads
    void rank_topn_run(long S, const unsigned *user, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value, const int64_t *ban_ptr,
                       const unsigned *ban_item, int top_n, int *item_out, float *score_out, int *count_out, int *nan_out, const RankLines *lines = nullptr);
    // the body of the top-N calls behind their validated lists (pieces, workspace, launches, copy-back); query_base: an item call
    void rank_topn_sweeps(const char *who, long S, const unsigned *sec_id, const RankTopnLists &L, const int64_t *fb_ptr, const unsigned *fb_index,
                          const float *fb_value, const RankLines *lines, const float *item_rows, const float *item_bias, const float *query_base,
                          int top_n, int *item_out, float *score_out, int *count_out, int *nan_out);
    // similar-item lists on the live model: dot and cosine top-N per query item (svdf_itemtopn.cpp, svdf_k_itemrows.hip)
    void item_topn(long S, const unsigned *item, int metric, const int64_t *ban_ptr, const unsigned *ban_item, int top_n, int *item_out,
                   float *score_out, int *count_out, int *nan_out);
    // the same rankings over per-section candidate lists instead of the catalogue minus bans (svdf_rankcand.cpp, svdf_k_rankcand.hip; DESIGN.md
    // section 6aa).  Exactly one of user / U.ptr is set; top_n == 0: positions (pos_*, position_out, tied_out, ranked_out), else the top_n lists
    void rank_cand(const char *who, long S, const unsigned *user, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                   const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *cand_ptr, const unsigned *cand_item, int top_n, int *position_out,
                   int *tied_out, int *ranked_out, int *item_out, float *score_out, int *count_out, int *nan_out);
    // positions over the positives and num_neg negatives the device draws per section from (seed, section, what the section excludes)
    // (svdf_ranknegs.cpp, svdf_k_ranknegs.hip).  Exactly one of user / U.ptr is set; neg_out may be nullptr
    void rank_negs(long S, const unsigned *user, const RankLines &U, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                   const int64_t *pos_ptr, const unsigned *pos_item, const int64_t *ban_ptr, const unsigned *ban_item, int num_neg, uint64_t seed,
                   int *position_out, int *tied_out, int *ranked_out, int *nan_out, int *neg_out);

    // passes of rank pairs from positives only, the negatives drawn on the device (svdf_pairsource.cpp, svdf_k_pairdraw.hip; DESIGN.md
    // section 6ac).  A source belongs to the handle it was created on and may outlive it.
    PairSource *pair_source_create(long n, const unsigned *user, const unsigned *pos, const unsigned *item_weight = nullptr);
    void pair_weight_lookup(long num_item, const unsigned *item_weight, int form, long nx, const uint64_t *x, unsigned *id_out);   // test probe (svdf_pair_weight_lookup): the map on the device
    // num_cand = 0: the plain pass; >= 1: the hard pass, the best of num_cand candidates by live score
    // order: the order_seed of a shuffled pass (section 6af), nullptr for the source's own order; the shuffled draw also returns the pass's
    // user and item columns [n * num_neg]
    Dataset *dataset_from_pair_source(PairSource *src, int num_neg, uint64_t seed, int num_cand = 0, const uint64_t *order = nullptr);
    void pair_source_draw(PairSource *src, int num_neg, uint64_t seed, unsigned *neg_out, int num_cand = 0, float *score_out = nullptr,
                          const uint64_t *order = nullptr, unsigned *user_out = nullptr, unsigned *pos_out = nullptr);
    void pair_source_forget(PairSource *src);   // (the source is being destroyed)

    // multi-GPU item-side delta
    // the per-rank exchange entry points (one process per GPU) make no sense on a handle that exchanges by itself
    void per_rank_api() const {
        if (multi_ && !in_multi_scope())
            fail("svdfeature_amd: svdf_item_delta_* / svdf_window_delta_* / svdf_item_block_* are the per-rank entry points of the one-process-per-GPU "
                 "scheme; an amd:gpus > 1 handle exchanges by itself (train through svdf_update* / svdf_train_dataset)");
    }
    void item_delta_begin();
    void *item_delta_buffer(int64_t *count);
    void item_delta_apply();
    void item_delta_copy(float *device_dst, const float *device_src);
    void item_delta_into(float *device_dst, int64_t *count);
    void item_delta_apply_from(const float *device_src);
    void item_delta_select(int part, int nparts);                              // active exchange partition (item id ranges)
    void item_delta_pack(void *device_dst, int half, int64_t *count);          // one launch, fp32 or fp16 wire format
    void item_delta_unpack(const void *device_src, int half, int refresh_snapshot);
    void set_stream(hipStream_t s);

    // introspection
    int64_t get_view(int which, float *out, int64_t capacity);
    int64_t set_view(int which, const float *in, int64_t count);
    void view_shape(int which, int *rows, int *cols);
    hipStream_t stream() const { return stream_; }
    std::string path_for(const Dataset *ds) const;   // the schedule form + kernel family a resident data set takes (svdf_dataset.cpp)
    void note_dataset(Dataset *ds);                  // once per data set from the C entry points: the default-step guard (counters 26 .. 28)
    void synchronize();
    int64_t counter(int what) const;
    int set_knob(const char *name, long value);
    void flush();

  private:
    // ---- configuration
    TypeParam mtype_;
    ModelParam mp_;
    TrainParam tp_;
    ParamSet u_param_, i_param_, g_param_;
    std::string name_feat_user_ = "NULL", name_feat_item_ = "NULL";
    SideTable feat_user_, feat_item_;
    int round_counter_ = 0;
    bool space_allocated_ = false, trainer_ready_ = false;
    // ---- geometry (SVDModel::alloc_space, apex_svd_model.h:511-556)
    int pitch_ = 0;
    static int row_pitch(int num_factor) { return ((num_factor + 3) / 4) * 4; }   // floats of a factor row: ceil(4k/16)*16 bytes (apex_tensor_sse.h:26-27)
    long n_uiset_ = 0;
    unsigned user_off_ = 0, item_off_ = 0, fb_off_ = 0;
    int num_fb_rows() const { return mp_.common_feedback_space == 0 ? mp_.num_ufeedback : mp_.num_user; }
    bool user_group() const { return mtype_.format_type == 1; }
    void compute_geometry();
    // ---- host model (only between init/load and upload, or transiently for save/get_view)
    std::vector<float> hW_, hbias_, hg_;
    bool host_model_valid_ = false;
    void alloc_host_model();
    void rand_init();
    bool rand_init_device();
    void upload_model();
    void download_model();
    void read_model(FILE *fi);
    void read_model_to_device(FILE *fi);
    void file_to_dev(FILE *fi, float *ddst, long rows, long cols, long pitch);
    void write_model(FILE *fo);
    // ---- device
    int device_ = -1;
    bool host_only_ = false;
    hipStream_t stream_ = nullptr;
    bool owns_stream_ = true;
    DevBuf<float> dW_, dbias_, dg_, dstate_;
    bool device_model_ = false;
    DevBuf<unsigned> d_ubound_, d_ibound_, d_gbound_, d_fu_ptr_, d_fu_idx_, d_fi_ptr_, d_fi_idx_;
    DevBuf<float> d_uwd_, d_iwd_, d_gwd_, d_fu_val_, d_fi_val_;
    DevParams dev_params_;
    bool params_dirty_ = true;
    const DevParams &params();
    void need_device(const char *what);
    // ---- staging + scheduling
    HostCSR staged_;
    struct HostUnit { int fb_begin, fb_end, row_begin, row_end, flags; };
    std::vector<HostUnit> staged_units_;
    std::vector<unsigned> staged_fb_index_;
    std::vector<float> staged_fb_value_;
    // extend_type 2 (SVDPPMultiIMFB, solvers/multi-imfb/apex_multi_imfb.h): blocks + units over block ranges, depth = the
    // reference's `top` after everything staged or issued so far
    bool imfb() const { return mtype_.extend_type == 2; }
    std::vector<DevBlk> staged_blks_;
    std::vector<DevUnit> staged_iunits_;
    int imfb_depth_ = 0;
    bool iunit_open_ = false;
    unsigned imfb_disable_ = 0;
    bool imfb_deep_ = false;   // the data nested deeper than IMFB_DEPTH levels at some point: launches use the IMFB_DEPTH_MAX build of k_imfb
    void update_block_imfb(int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row, const float *row_label,
                           const int *row_ptr, const unsigned *feat_index, const float *feat_value);
    void schedule_iunits(int base, Schedule &sched);
    void upload_iunits(UnitDev &dst, const Schedule &sched);
    void flush_iunits();
    void drop_staged_units();
    // extend_type 15 (SVDBiLinearTrainer, solvers/bilinear/apex_svd_bilinear.h): BParam + W_bi travel with the model file
    bool bilinear() const { return mtype_.extend_type == 15; }
    struct BiParam { int num_bi_feedback, start_ufeedback, reserved[32]; } bi_param_;
    std::vector<float> hbi_;
    bool bi_allocated_ = false;
    int reg_bi_feedback_ = 0;
    bool unit_open_ = false;          // a START block was staged and its END has not arrived
    bool unit_open_on_device_ = false;  // ... and its first part was already flushed (state saved on device)
    long stage_window_ = 1 << 21;   // rows per staged window: 1-4 M measure alike in tools/update_call_cost (125-153 M inst/s), smaller windows end a round sooner
    bool use_graph_ = false;   // measured: no gain, dependent short kernels are bound on the GPU side
    int graph_min_levels_ = 2;
    uint64_t launch_version_ = 1;
    std::vector<unsigned char> staged_fresh_;   // per staged row, see DevCSR::row_fresh
    bool any_fresh_ = false, simple_unit_values_ = false;
    // relaxed mode for shared ids (extension keys "amd:relax_global", "amd:relax_user_from", "amd:relax_item_from")
    bool relax_global_ = false, relax_feedback_ = false;
    int g_stride_ = 1;                  // device layout of g_bias, see DevParams::g_stride
    int wanted_g_stride() const { return (relax_global_ && mp_.num_global <= (1 << 24)) ? 32 : 1; }
    void upload_globals(int stride);
    void download_globals(float *dst);
    unsigned relax_user_from_ = 0xFFFFFFFFu, relax_item_from_ = 0xFFFFFFFFu;
    // extension key "amd:shared_user_from" = B (one GPU, window step only): user ids >= B are shared attribute rows, moved like item rows
    unsigned shared_user_from_ = 0xFFFFFFFFu;
    bool shared_user() const { return shared_user_from_ != 0xFFFFFFFFu; }
    // what `auto` may hand to the window step as shared ids (wunit_rows_ok): none when their refusals would apply (bf16 contribution rows)
    unsigned shared_user_for_auto() const { return shared_user() && !contrib_bf16_ ? shared_user_from_ : 0xFFFFFFFFu; }
    PairSampler pair_sampler_;
    RankPrefetch *rank_prefetch_ = nullptr;
    std::vector<Dataset *> datasets_;     // live datasets of this trainer (Dataset::owner back-pointers)
    void adopt(Dataset *ds);
    // device-side scheduling of column-shaped data sets (svdf_k_sched.hip): ucols / fcols = (host column in file order, destination
    // buffer in level order); res_col[s] = index into ucols of slot s's id column
    struct UCol { const unsigned *src; DevBuf<unsigned> *dst; };
    struct FCol { const float *src; DevBuf<float> *dst; };
    void schedule_columns_on_device(Dataset *ds, long n, int K, const int *res_col, const unsigned *off, const unsigned *limit,
                                    const char *const *msg, int sort_col, unsigned sort_max, const std::vector<UCol> &ucols, const std::vector<FCol> &fcols);
    const int *host_order(Dataset *ds);
    bool device_sched_ = true;            // knob "device_schedule"
    long device_sched_min_ = 1 << 16;     // staged windows smaller than this stay on the host scheduler (knob "device_schedule_min")
    Dataset w_dataset_;                   // schedule scratch of device-scheduled staging windows (never adopted)
    uint64_t schedule_signature() const;
    void disown(Dataset *ds);
    void rank_pass(const char *path, UserGroupArrays &g);
    // nullptr when the file or the sampler settings need the host path.  as_windows: the drawn columns become a window sequence (kind 8 of kind-5
    // pair windows, wseq_from_device_pairs) instead of an exact level-scheduled pass (kind 2); nullptr also when the windows do not take the pass
    Dataset *rank_pass_device(const char *path, bool as_windows = false);
    bool rank_window_route_ok() const;             // what the configuration must satisfy for as_windows (the file's part: RankSource::unit_values)
    bool rank_source_load(const char *path);       // (re)loads rank_source_ for this file; false when it cannot be opened / stat'ed
    bool rank_pass_device_general(const char *path, UserGroupArrays &g);   // any row shape / method: the pass drawn in HBM, blocks back in g
    std::unique_ptr<RankSource> rank_source_;
    bool device_rank_ = true;                       // knob "device_rank"
    bool device_load_ = true;                       // knob "device_load": load_model streams the matrices file -> pinned chunks -> HBM (0 = through a host copy of the model)
    bool device_window_ = true;                     // knob "device_window": kind-5 window data sets regrouped on the device (svdf_k_wbuild.hip)
    bool device_init_ = true;                       // knob "device_init": rand_init on the device (svdf_k_init.hip)
    int device_init_margin_log2_ = 46;              // knob "device_init_margin_log2": values closer than 2^-this (relative) to a float rounding boundary go to the host libm
    int64_t n_init_reports_ = 0, n_init_draws_ = 0, n_chained_levels_ = 0;
    long chain_width_ = 128;                        // knob "chain_width": levels of at most this many instances are walked in runs inside ONE launch by one workgroup (0 = off)
    bool fewrow_fast_ = true;                       // knob "fewrow_fast": specialised few-row kernel (svdf_k_fewrow.hip)
    // columns that are already in HBM (file order) -> level schedule + level-sorted copies
    Dataset *dataset_fewrow_on_device(long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    struct DUCol { const unsigned *src; DevBuf<unsigned> *dst; };
    struct DFCol { const float *src; DevBuf<float> *dst; };
    void schedule_device_columns(Dataset *ds, long n, int K, const unsigned *const *res_col, const unsigned *off, const unsigned *limit,
                                 const char *const *msg, const unsigned *sort_key, unsigned sort_max, const std::vector<DUCol> &ucols,
                                 const std::vector<DFCol> &fcols);
    bool rows_without_feedback_ = true;   // knob: block datasets without any feedback id are scheduled row by row
    bool rows_as_instances_ = false;      // set while such a dataset is being built
    bool relaxed() const { return relax_global_ || relax_feedback_ || relax_user_from_ != 0xFFFFFFFFu || relax_item_from_ != 0xFFFFFFFFu; }
    // lazy decay modes (apex_svd_base.h:95-97,157-170): the reference's sample_counter and per-id ref words
    unsigned sample_counter_ = 0;
    DevBuf<unsigned> d_ref_ui_, d_ref_global_;
    bool lazy_decay() const { return tp_.reg_method >= 4 || tp_.reg_global >= 4; }
    int groups_per_wave_ = 0, block_threads_ = 0, store_mode_ = 0, load_mode_ = 2, basic_i8_ = 1, svdpp_helpers_ = 8, svdpp_xunits_ = 1, small_blocks_ = 1, fewrow_i16_ = 1, sort_batches_ = 1, xcd_remap_ = 1, hot_reduce_ = 1;   // 0 = tuned per factor width
    LevelTracker tracker_;
    void stage_rows(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value);
    void stage_rows_into(HostCSR &dst, int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value);
    void check_row(int ng, int nu, int ni, const unsigned *index);
    bool basic_fast_path_allowed() const;
    bool window_rows_allowed() const;     // the same with the width bound at 1024: what the window kernels of ratings / rank pairs take
    bool fused_allowed() const;
    bool fused_allowed_for_rows() const;   // the same for the rows of a feedback-free user-group pass
    template <typename PtrT> bool fused_shape_ok(long n, const PtrT *row_ptr, const unsigned *idx, FusedHost &out);
    template <typename PtrT> void fill_fused(long n, const float *row_label, const PtrT *row_ptr, const unsigned *idx, const float *val,
                                             const int *order, FusedHost &out);
    FusedHost w_fused_host_;
    FusedDev w_fused_;
    bool use_fused_ = true, use_simple_units_ = true;
    size_t num_resources() const { return (size_t)n_uiset_ + (size_t)mp_.num_global; }
    // per-unit level assignment
    int level_of_row(const unsigned *ig, int ng, const unsigned *iu, int nu, const unsigned *ii, int ni, int lvl0);
    void touch_row(const unsigned *ig, int ng, const unsigned *iu, int nu, const unsigned *ii, int ni, int lvl);
    void flush_csr(HostCSR &src);
    void flush_units();
    // background flush of full windows (random-order trainers only)
    void submit_window();
    void wait_worker();
    void worker_main();
    std::thread worker_;
    std::mutex mu_;
    std::condition_variable cv_;
    HostCSR job_;
    bool worker_busy_ = false, worker_stop_ = false, async_flush_ = true;
    std::string worker_error_;
    // levels + DevUnit records for the staged units (marks UNIT_SIMPLE); returns the schedule
    void schedule_units(int base, Schedule &sched, std::vector<DevUnit> &du);
    void upload_unit_arrays(UnitDev &dst);
    void upload_units(UnitDev &dst, const Schedule &sched, const std::vector<DevUnit> &du, bool scheduled_on_device = false);
    bool schedule_units_on_device(UnitDev &dst, Schedule &sched, std::vector<DevUnit> &du);
    int64_t unit_sched_us_ = 0;
    bool unit_sched_on_device_ = false;   // resident user-group data sets (svdf_k_sched.hip)
    std::vector<int64_t> stamp_;   // scratch for per-unit distinctness checks: stamp_epoch_ + unit index of the last toucher
    int64_t stamp_epoch_ = 0;
    // reusable device staging buffers
    DevBuf<float> w_label_, w_value_, w_uval_, w_ival_, w_fbval_, w_out_, w_pred_;
    DevBuf<int> w_ptr_, w_order_;
    DevBuf<unsigned> w_index_, w_user_, w_item_, w_fbidx_;
    DevBuf<DevUnit> w_units_;
    UnitDev w_unitdev_;
    // ---- item delta
    DevBuf<float> d_snap_, d_delta_;
    // scratch of the device window builder (svdf_k_wbuild.hip), grow-only: the window's columns as handed over + sort / scan buffers
    DevBuf<unsigned> wb_user_, wb_item_, wb_neg_, wb_k0_, wb_k1_, wb_v0_, wb_v1_, wb_inst_, wb_state_;
    DevBuf<float> wb_label_;
    DevBuf<int> wb_slot_e_, wb_head_, wb_mark_, wb_run_user_, wb_run_start_, wb_run_begin_;
    DevBuf<char> wb_tmp_;
    bool window_build_device(Dataset *ds, long n, const unsigned *user, const unsigned *item, const float *label, const unsigned *neg);
    void window_build_resident(Dataset *ds, long n, const unsigned *d_user, const unsigned *d_item, const float *d_label, const unsigned *d_neg);
    void window_build_header(Dataset *ds, long n, bool pairs, bool rows_as_instances = false);
    // scoring of window data sets (svdf_dataset.cpp): one window's predictions in regrouped order (pos == nullptr) or
    // scattered to out[pos[r]]; returns the window's labels in regrouped order (rank pairs: ones)
    const float *window_score(Dataset *c, float *out, const int *pos);
    void window_score_reserve(Dataset *const *child, size_t nchild);
    bool staged_building_ = false;        // set while a staged chunk's transient window sequence is built (svdf_staged.cpp): no file positions
    bool window_keeps_positions() const { return !staged_building_ && !in_multi_scope(); }
    DevBuf<unsigned> w_ucol_;             // scoring scratch: the user (kind 7: + segment) of every regrouped row of the window being scored
    DevBuf<int> w_segcol_;
    DevBuf<float> w_sfb_, w_sfbb_, w_ones_;   // ... the segments' prepared feedback sums / biases (kept apart from d_dvec_: a trained window's pending sums read that), labels of rank pairs
    bool device_window_ready() const { return !host_only_ && device_window_; }
    DevBuf<float> d_dvec_, d_dbias_;      // deferred feedback scatter: one scaled delta row + bias delta per segment of the largest window
    DevBuf<float> d_hfb_, d_hfbb_;        // user-group windows with hot shared user rows (window_block_sub) or hot item rows (window_block_item_sub): tmp_ufeedback + its bias per hot record of the largest window
    DevBuf<float> d_contrib_, d_cbias_;   // window-minibatch scratch: one contribution row + bias word per instance of the largest window
    std::unique_ptr<IpcState, IpcDeleter> ipc_;
    std::unique_ptr<RcclState, RcclDeleter> rccl_;
    void rccl_check(const char *what);
    void ipc_check(const char *what);
    DevBuf<float> d_gcontrib_;            // ... and one word per global entry (user-unit windows)
    // user-unit windows (svdf_wunit.cpp)
    WUnitSchedule wunit_view(const Dataset *ds) const;
    // side_tables: the caller is the one-GPU window sequence of random-order rows (wseq_from_csr), which takes feature_user / feature_item
    // children as shared rows; every other window builder refuses loaded side tables
    void wunit_check_config(const char *what, bool side_tables = false) const;
    bool side_tables() const { return feat_user_.num_row() != 0 || feat_item_.num_row() != 0; }
    void side_children_ok(const int64_t *row_ptr3, const unsigned *feat_index, std::vector<unsigned> &seen) const;   // svdf_wunit.cpp
    const char *side_children_rule(const int64_t *row_ptr3, const unsigned *feat_index, std::vector<unsigned> &seen) const;
    bool wunit_width_ok() const;        // the user-unit kernels' width (one lane group per row): the sub-step lanes, the N-rank builders, the staged route, `auto`
    bool wunit_wide_ok() const;         // the one-GPU window sequence of user units (wseq_from_csr / wseq_from_blocks): wide rows too, a wave per unit
    bool wunit_config_ok(bool user_units = true) const;       // the same conditions as a predicate (svdf_multi.cpp picks the step per data set)
    void wunit_build_host(WUnitHost &H, bool inplace, const void *segs, size_t nseg, const std::vector<int64_t> &seg_rows, bool by_row_order, long num_src_row,
                          const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value,
                          const unsigned *fb_index, const float *fb_value, const int64_t *priv_pos = nullptr, bool children = false, int shared_sub = 0, int item_sub = 0) const;
    void wunit_adopt(Dataset *ds, const WUnitHost &H);
    void wunit_host_from_csr(WUnitHost &H, bool inplace, long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value,
                             bool shared = false, int shared_sub = 0, int item_sub = 0) const;
    void wunit_host_from_blocks(WUnitHost &H, bool inplace, long b0, long b1, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value,
                                bool shared = false, int shared_sub = 0, int item_sub = 0) const;
    int wseq_build_threads_ = 32;         // knob "wseq_build_threads": host threads building the windows of a one-GPU window sequence (user units)
    int64_t private_user_entry(int64_t p1, int64_t p2, const unsigned *feat_index, std::vector<unsigned> &seen) const;   // amd:shared_user_from: the one id < B of a row's user entries
    void wunit_train(Dataset *ds);
    void wunit_sum(Dataset *ds, void *dst, int half);
    // one GPU, `amd:step = minibatch` (opt-in; not the reference's semantics): resident data sets become window sequences (kind 8)
    bool step_minibatch_set_ = false;
    bool contrib_bf16_ = false;           // "amd:contrib = bf16": contribution rows of the window-minibatch step in bfloat16 (opt-in)
    int fewrow_gslots_ = 1;               // knob "fewrow_gslots": 0 = k_fused for few-row data sets with inline global slots (A/B)
    int wunit_defer_fb_ = 1;              // knob "wunit_defer_fb": feedback-row contributions are formed by k_wunit_sum from the segments' deltas (1) or written as rows by the walk (0: A/B; same bits)
    int wunit_inplace_ = 1;               // knob "wunit_inplace": one-GPU window sequences apply a row's only contribution of a window in place (no slot); 0 = every contribution through a slot (A/B)
    int wunit_fast_ = 2;                  // knob "wunit_fast": 0 = the general lane-group kernel for every shape, 1 = + the slot kernel, 2 = + one wave per unit, 3 = + its form for user-group windows with shared user entries (A/B and tests)
    int wseq_per_target_fb_ = 16;         // knob "window_per_target_fb": the same for feedback rows (instance-sized updates pushed by whole blocks)
    int wseq_per_target_child_ = 3;       // knob "window_per_target_child": the same for side-table children (calibrated on the
                                          // variant of profiles/r08_sidetable_window.md, 3 seeds at 2 M rows: 12 -> |dRMSE| 2.2e-4, 6 -> 1.1e-4, 4 -> 8.8e-5, 3 -> 5.7e-5)
    int wseq_per_target_shared_ = 12;     // knob "window_per_target_shared": the same for shared user rows (amd:shared_user_from; calibrated on the
                                          // SURVEY 8(d2) variant, 3 seeds: 24 -> |dRMSE| 1.3e-4, 16 -> 1.1e-4, 12 -> 6.1e-5; profiles/r07_sidefeat_window.md)
    int wseq_per_target_max_ = 128;       // knob "window_per_target_max": the MOST updates any shared row may meet per window (binds on skewed data only)
    // ordered sub-steps for hot items of a one-GPU window sequence of plain ratings (svdf_k_window.hip: k_window_apply; round 6)
    int wseq_shared_sub_ = 0;             // knob "window_shared_sub": a shared user row (id >= amd:shared_user_from, feature_user children included) with more slots than this in a window of wseq_from_csr is applied in ordered sub-steps of this many (k_wunit_apply_shared); 0 = off
    int wseq_shared_max_ = 512;           // knob "window_shared_max": the most updates a hot shared user row may meet per window (how stale everybody else's view of it gets); side-feature variant at the 20 M-row prefix, window_shared_sub 12, 3 seeds: 256 max |dRMSE| 7.2e-5 / 191 ms per pass, 512 6.9e-5 / 172 ms, 1 024 1.06e-4 (profiles/r09_shared_hot.md)
    int wseq_item_sub_ = 0;               // knob "window_item_sub" (0 .. 128): an item-range row (a plain item entry's row, a feature_item child's row) with more slots than this in a window of wseq_from_csr is applied in ordered sub-steps of this many (k_wunit_apply_hot<ITEM>); 0 = off
    int wseq_item_max_ = 2048;            // knob "window_item_max": the most updates a hot item row may meet per window (how stale everybody else's view of it gets); the largest swept value: Zipf(0.7) items + 4 globals, 2 M rows, 3 seeds, sub 8 / 24 / 128: max |dRMSE| 6.0e-6 / 2.3e-6 / 2.2e-5 (profiles/r11_item_hot.md)
    int wseq_block_sub_ = 0;              // knob "window_block_sub" (0 .. 4096): a shared user row with more slots than this in a window of user-group blocks (wseq_from_blocks under amd:shared_user_from) is applied in ordered sub-steps of this many (k_wunit_apply_hot<LPI, false, true>); 0 = off
    int wseq_block_max_ = 512;            // knob "window_block_max": the most updates a hot shared user row of such blocks may meet per window; taken over from window_shared_max and NOT confirmed: on 64 dense buckets (2 M rows, 3 seeds) no cap of 128 .. 1 024 holds |dRMSE| <= 1e-4, nor does the rule with the knob off (profiles/r16_block_hot.md)
    int block_sub() const { return user_group() && shared_user() ? wseq_block_sub_ : 0; }   // the knob as it takes effect: user-group trainers with amd:shared_user_from
    void wseq_block_check(const char *what) const;   // window_block_sub in effect: what the lane does not cover, refused with its cause
    int wseq_block_item_sub_ = 0;         // knob "window_block_item_sub" (0 .. 128): an item row with more slots than this in a window of user-group blocks (wseq_from_blocks) is applied in ordered sub-steps of this many (k_wunit_apply_hot<LPI, true, true>); 0 = off
    int wseq_block_item_max_ = 2048;      // knob "window_block_item_max": the most updates a hot item row of such blocks may meet per window; taken over from window_item_max; holds |dRMSE| <= 1e-4 on Zipf(0.7) items over 2 M rows of SVD++ blocks (3 seeds, sub 64 / 128: at most 5.9e-5; profiles/r22_block_item_hot.md).  4 096 holds it too but cut the same 14 windows there (the feedback term binds; the hottest item meets about 1 400 updates per window), so it was not taken: the largest cap exercised as a bound is 1 024
    int block_item_sub() const { return user_group() ? wseq_block_item_sub_ : 0; }   // the knob as it takes effect: user-group trainers (their passes are in file order), with or without amd:shared_user_from
    void wseq_block_item_check(const char *what) const;   // window_block_item_sub in effect: what the lane does not cover, refused with its cause
    int wseq_pair_sub_ = 0;               // knob "window_pair_sub" (0 .. 128): an item with more slots than this (both signs counted) in a window of rank pairs (wseq_from_pairs) is applied in ordered sub-steps of this many (k_window_apply_pairs); 0 = off
    int wseq_pair_max_ = 4096;            // knob "window_pair_max": the most updates a hot item of rank pairs may meet per window (how stale everybody else's view of it gets); the largest swept value: Zipf(0.7) pairs at the configs[4] shape, 20 M-pair prefix, 3 seeds, sub 8 / 24 / 128: worst seed at 3 % of the pair contract (accuracy within 3e-3, margin within 2 %; profiles/r12_pair_hot.md)
    int wseq_hot_sub_ = 128;              // knob "window_hot_sub": an item with more slots than this in a window is applied in sub-steps of this many (0 = off: the round-5 rule, no row more than window_per_target_max per window)
    int wseq_hot_max_ = 2048;             // knob "window_hot_max": the most updates a hot row may meet per window (how stale the USERS' view of it gets); 3 seeds of Zipf(0.7) at the configs[1] size: 1 024 max |dRMSE| 4.2e-5 / 66 ms per pass, 2 048 6.6e-5 / 55 ms, 3 072 7.2e-5 / 52 ms (profiles/r06_hot_lane_calibration.txt)
    DevBuf<float> d_clabel_;
    int wseq_count_actual_ = 1;           // knob "window_count_actual": 1 = the window rule is evaluated on the windows as they are cut and W raised until it holds (svdf_wseq_rule.h: wseq_actual_columns / _csr); 0 = the per-pass rule alone
    WseqKnobs wseq_knobs() const;         // the knob values the window rule reads (svdf_wseq_rule.h), amd:window among them
    bool wseq_hot_ok() const;             // the configuration has the hot lane (unit ratings, fp32 contribution rows, one GPU)
    void resident_rows_check() const;               // what dataset_from_csr (and every caller that ends there) refuses about a user-group trainer
    void wseq_pair_check(const char *what) const;   // window_pair_sub > 0: what the lane does not cover, refused with its cause
    // the refusals common to the sub-step knobs (window_shared_sub, window_item_sub, window_pair_sub) when `knob` is on
    void wseq_sub_check(const char *what, const char *knob, const char *desc, const char *entry, const char *nrank, bool entry_only = false) const;
    std::vector<long> wseq_item_counts(long n, const unsigned *item, const unsigned *item1) const;
    Dataset *wseq_from_columns(long n, const unsigned *user, const unsigned *item, const unsigned *item1, const float *label,
                               const std::vector<long> &item_count, WseqLane lane);   // the body of wseq_from_triples / _pairs
    void wseq_count_targets(WseqCounts &C, long r0, long r1, const int64_t *row_ptr, const unsigned *feat_index) const;
    void wseq_adopt_window(Dataset *ds, const WUnitHost &H, long first);
    int wseq_per_target_ = 24;            // knob "window_per_target": updates a shared row meets per window when amd:window is not given
    bool single_minibatch() const { return step_minibatch_set_ && gpus_ == 1 && !multi_ && !is_peer_; }
    // runs of an item's consecutive ratings as the units of the contract workload's schedule (svdf_runs.cpp / svdf_k_runs.hip)
    int runs_exec_ = 1;                   // knob "runs_exec"
    int runs_len_ = 4;                    // knob "runs_len": ratings per run at most (2 .. 7)
    int runs_sets_ = 1, runs_block_ = 64; // knobs "runs_sets" / "runs_block": row sets per wave, threads per workgroup of k_basicmf_runs_soa
    long runs_min_rows_ = 1 << 20;        // knob "runs_min_rows": smaller data sets keep the plain schedule (levels too narrow for runs to matter)
    int runs_order_ = 1;                  // knob "runs_order": a level's runs sorted by 1 = (length, longest first; item), 0 = item; read when a data set is built, with sort_batches = 1
    int64_t n_runs_passes_ = 0;
    void runs_order_stats(Dataset *ds);
    bool runs_config_ok() const;
    Dataset *runs_dataset_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    void runs_train(Dataset *ds);
#ifdef SVDF_RUNS_STAMPS
    bool runs_probe_pass(Dataset *ds, const DevParams &P, RunSchedule &S);   // timing build: one stamped pass (svdf_runs.cpp)
#endif
    int runs_stage_ = 1;                  // knob "runs_stage": 1 = a run's rows are written into their next reader's schedule slot (where the gate allows), 0 = rows live in W
    int runs_store_ = 1;                  // knob "runs_store": how the staged runs kernel stores: 0 plainly, 1 the bias words nontemporal, 2 rows and bias words sc1 write-through
    long runs_stage_max_mb_ = -1;         // knob "runs_stage_max_mb": cap on a data set's staging buffers (-1: half of the free device memory is the only limit)
    void runs_stage_build(Dataset *ds);
    bool runs_staged(const Dataset *ds) const { return runs_stage_ != 0 && ds->rn_stage_state == 1 && ds->rn_stage_row0 == user_off_; }
    // exact passes over data with hot rows: runs of a hot row's ratings as walker units (svdf_pivot.cpp)
    int pivot_exec_ = 1;                  // knob "pivot_exec"
    int pivot_run_ = 256, pivot_run_long_ = 256;   // knobs "pivot_run" / "pivot_run_long": ratings per unit at most, among cold levels / beyond them (a longer tail cap measured slower)
    int pivot_min_ = 2048;                // knob "pivot_min": a row with at least this many ratings in the data set is hot
    int64_t n_pivot_passes_ = 0;
    // user-run units of rank pairs (svdf_punit.cpp; knob "pair_units", default on; "pair_unit_cap": pairs per unit at most)
    int pair_units_ = 1, pair_unit_cap_ = 16;
    int64_t n_punit_passes_ = 0;
    bool punit_config_ok() const;
    Dataset *punit_dataset_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg);
    bool punit_build(long n, const unsigned *user, const unsigned *lo, const unsigned *hi, std::vector<PairUnit> &sorted, std::vector<long> &level_ptr) const;
    bool punit_flush(HostCSR &src);        // a staged window of user-grouped rank pairs (the per-instance route of the reference CLI)
    DevBuf<PairUnit> w_pu_units_;
    PairUnitSchedule punit_view(const Dataset *ds) const;
    void punit_train(Dataset *ds);
    void punit_predict(Dataset *ds, float *d_out);
    bool pivot_config_ok() const;
    Dataset *pivot_dataset_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    void pivot_train(Dataset *ds);
    // one GPU, `amd:step = auto` (opt-in): every resident data set is level-scheduled first (that is cheap on the device); when the
    // dependency depth of exact sequential semantics -- levels x the latency of one unit -- exceeds twice what the pass would take at the
    // streaming rate, the data set is rebuilt as a window sequence (the contract of `amd:step = minibatch`), else the exact levels stay.
    bool step_auto_set_ = false, auto_building_ = false;
    struct AutoDecision { int decided = 0; long levels = 0, windows = 0; double dag_ms = 0.0, stream_ms = 0.0; } auto_last_;
    bool auto_step_active() const { return step_auto_set_ && !auto_building_ && gpus_ == 1 && !multi_ && !is_peer_ && !host_only_; }
    Dataset *auto_step(Dataset *exact, bool window_ok, const std::function<Dataset *()> &build_window);
    static constexpr long AUTO_PROBE_ROWS = 2000000, AUTO_PROBE_MIN = 8000000;
    AutoDecision auto_probe_;
    std::string auto_rank_path_;          // rank-pair input: the candidate file whose passes the decision below was taken for
    int auto_rank_decision_ = 0;
    bool auto_probe_deep(Dataset *probe, long n_full);
    // ONE place that names the path a resident data set takes (kernel family, schedule form) and, in the DEFAULT (exact) step, runs the
    // estimator of `amd:step = auto` on it: when the data's dependency depth is predicted to cost more than 10 x the streaming model, one
    // stderr line says so and names `amd:step = auto` (svdf_dataset.cpp; counters 26 .. 28).  Called once per data set by the C entry points.
    int64_t n_guard_warnings_ = 0;
    AutoDecision guard_last_;
    Dataset *wseq_from_csr(long n, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    Dataset *wseq_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                              const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    Dataset *wseq_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    Dataset *wseq_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg);
    // the same sequence from a pass of rank pairs the device sampler left in HBM (merged item entries i0 / v0 / i1 of unit-value rows, file order):
    // counts, window rule and windows without the columns visiting the host (svdf_k_rankwin.hip).  nullptr: a pair the windows do not take
    // (positive and negative row of one item, an id out of range) -- the caller falls back to the route that reports it
    // d_v0 == nullptr: d_i0 / d_i1 ARE the positive and the negative item of every pair (a pair source's draw, section 6ac) and are cut as they are
    Dataset *wseq_from_device_pairs(long n, const unsigned *d_user, const unsigned *d_i0, const float *d_v0, const unsigned *d_i1);
    void wseq_train(Dataset *ds);
    WindowSchedule window_view(const Dataset *ds) const;
    Dataset *window_trained_ = nullptr;   // the window data set whose contributions the scratch holds
    int window_slots_ = 1, window_groups_ = 0;   // knobs "window_slots", "window_groups"
    int delta_part_ = 0, delta_nparts_ = 1;
    DevBuf<double> d_partials_;
    struct Range { float *base; long n; };
    std::vector<Range> shared_ranges();
    // ---- `amd:step = minibatch | auto` on the staged route of a one-GPU handle (svdf_staged.cpp): a chunk of staged
    // rows is trained as the window sequence svdf_dataset_from_* would build from it; chunks the window step does not cover keep the exact flush
    bool staged_step_wanted() const { return (step_minibatch_set_ || step_auto_set_) && gpus_ == 1 && !multi_ && !is_peer_ && !host_only_; }
    const char *staged_config_rule(bool blocks, bool user_units) const;   // nullptr: the configuration is inside the window step, else the rule that keeps it out
    bool staged_window_csr(HostCSR &src);                // true: the chunk was trained by the window step (src is cleared)
    bool staged_window_units();                          // the same for the closed units of a user-group trainer (flush_units)
    bool staged_window_live() const { return staged_step_wanted() && !auto_building_ && (!step_auto_set_ || staged_auto_decision_ == 0 || staged_auto_decision_ == 2); }
    bool staged_auto_decide(long n, int kind, long units, long levels, long bytes, const char *rule, const std::function<Dataset *()> &build_window, Dataset *&out);
    void flush_units_exact();                            // the level-scheduled unit flush (svdf_sched.cpp)
    void staged_train(Dataset *seq);                     // trains and drops a transient window sequence
    void staged_keep_exact(const char *rule);            // counter 31 and, once per handle, one stderr line naming the rule
    void staged_guard(long n, long levels, double unit_us, long bytes);   // the default step's guard for staged chunks (counter 32)
    struct StagedBlk { int tag, unit, row_begin, row_end; };   // unit: index into staged_units_
    std::vector<StagedBlk> staged_blks_w_;               // user-group trainers: the staged blocks as handed over (wseq_from_blocks cuts windows in blocks)
    int staged_auto_decision_ = 0;                       // amd:step = auto: 0 not taken yet, else auto_last_.decided of the chunk it was taken on
    int64_t n_staged_window_ = 0, n_staged_exact_ = 0, n_staged_guard_ = 0;
    int64_t n_block_hot_ = 0;                            // hot shared user rows applied in ordered sub-steps on user-group windows (counter 35)
    int64_t n_block_item_hot_ = 0;                       // hot item rows applied in ordered sub-steps on user-group windows (counter 36)
    int64_t n_wave_shared_ = 0, n_walk_shared_ = 0;      // user-group windows with shared user entries: walked by the wave form / by the general kernel (counters 33 / 34)
    int64_t ns_staged_build_ = 0;                        // host time of the per-chunk pre-check + window build (part of ns_flush_; SVDF_PROFILE prints it)
    int64_t ns_rank_draw_ = 0, ns_rank_rule_ = 0, ns_rank_wbuild_ = 0;   // rank passes built as device window sequences: wall time of the draw / of the item counts + window rule / of the windows' regrouping (SVDF_PROFILE prints it)
    int64_t ns_wseq_host_ = 0, ns_wseq_adopt_ = 0;       // user-unit window sequences (wseq_build_windows): wall time of the host regrouping / of the windows' allocations + uploads + synchronisations
    std::string staged_auto_rule_;                       // amd:step = auto, decision 3: the rule that keeps the chunks exact
    long staged_defer_factor_ = 4;                       // a user still open after this many stage_window rows no longer holds back the automatic flush
    bool staged_exact_said_ = false;
    DevPool staged_pool_;
    int staged_pool_mode_ = 1;                           // knob "staged_pool": 0 = hipMalloc / hipFree per chunk (A/B; same bits), 1 = the handle's pool
    // ---- N GPUs behind this handle (svdf_multi.cpp)
    int gpus_ = 1;
    bool is_peer_ = false, delta_half_ = true, window_set_ = false;
    std::vector<std::pair<std::string, std::string>> param_log_;   // every set_param so far, replayed on the other ranks
    std::unique_ptr<MultiState, MultiDeleter> multi_;
    Engine *rank_engine(int d);
    void multi_setup();
    void multi_copy_model_to_peers();
    void multi_flush(HostCSR &src);
    void multi_prepare();
    void multi_window(const std::function<void(int, Engine *)> &train, bool minibatch, Dataset *const *mb);
    bool multi_minibatch_allowed() const;
    Dataset *multi_dataset_from_triples(long n, const unsigned *user, const unsigned *item, const float *label);
    Dataset *multi_dataset_from_pairs(long n, const unsigned *user, const unsigned *pos, const unsigned *neg);
    Dataset *multi_dataset_from_csr(long num_row, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index, const float *feat_value);
    Dataset *multi_dataset_from_blocks(long num_block, const int *extend_tag, const int64_t *fb_ptr, const unsigned *fb_index, const float *fb_value,
                                       const int64_t *block_row_ptr, const float *row_label, const int64_t *row_ptr, const unsigned *feat_index,
                                       const float *feat_value);
    void multi_train_dataset(Dataset *ds);
    void multi_synchronize();
    int multi_predict_rank_ = 0;         // owner of the user-group block scored last (predict_block on an amd:gpus handle)
    int multi_exchange_mode_ = 0;        // "amd:exchange": 0 p2p (peer loads / stores between the ranks of this process), 1 rccl
    bool multi_step_levels_ = false;     // "amd:step = levels": exact conflict-free levels per rank instead of the window-minibatch step
    std::unique_ptr<Dataset> w_window_;  // the staged path's window-minibatch data set of this rank, rebuilt in place every window
    void window_build(Dataset *ds, long n, const unsigned *user, const unsigned *item, const float *label, const unsigned *neg = nullptr);
    void multi_predict(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value, float *out);
    void multi_gather_user_rows();
    int64_t multi_counter(int what) const;
    void item_delta_begin_local();
    void predict_csr_batch_local(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value, float *out);
    // ---- counters
    int64_t n_instances_ = 0, n_launches_ = 0, n_batches_ = 0, n_flushes_ = 0;
    static constexpr size_t PRED_PIN_WORDS = 1 << 16;   // predict of a few rows: pinned, device-mapped staging (rows in, predictions out)
    unsigned *pred_pin_ = nullptr;
    // save_model: pinned double buffer of the device -> file pipeline, one for the synchronous path and one for the writer thread of the asynchronous one
    static constexpr size_t SAVE_PIN_FLOATS = (size_t)8 << 20;
    struct SavePipe { float *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; hipStream_t st = nullptr; };
    SavePipe save_pipe_;
    struct SaveAsync { DevBuf<float> W, bias; std::vector<float> g; hipEvent_t ready = nullptr; hipStream_t st = nullptr; SavePipe pipe; std::thread th;
                       std::string error; bool active = false; } save_async_;
    void save_pipe_init(SavePipe &sp, hipStream_t st);
    static void save_pipe_free(SavePipe &sp);
    void dev_to_file(SavePipe &sp, FILE *fo, const float *dsrc, long rows, long cols, long pitch);
    void write_model_from_device(SavePipe &sp, FILE *fo, const float *W, const float *bias, const float *g);
    void write_model_from_device(FILE *fo);
    int64_t ns_flush_ = 0, ns_model_ = 0;   // host-side time accounting (SVDF_PROFILE=1 prints it)
    int64_t n_device_rank_passes_ = 0;
    int64_t n_rank_window_passes_ = 0;   // counter 37: rank passes built as device window sequences
    int64_t n_rank_eval_sections_ = 0;   // counter 38: sections ranked by the batch evaluation's sweep
    long rank_eval_budget_ = 1L << 22;   // knob rank_eval_budget: positives + distinct bans + sections of one piece
    DevBuf<int> re_in_, re_cnt_;
    DevBuf<float> re_ps_;
    int64_t n_rank_topn_sections_ = 0;   // counter 39: sections listed by svdf_rank_topn
    long rank_topn_budget_ = 1L << 25;   // knob rank_topn_budget: 64-bit keys of the list workspace of one piece (256 MiB)
    DevBuf<int> tn_in_, tn_out_;
    DevBuf<unsigned long long> tn_list_;
    int64_t n_rank_fb_sections_ = 0;   // counter 40: sections the _fb calls ranked with a row built from a feedback list
    DevBuf<float> rk_rows_;            // a piece's effective user rows, [nsec][pitch]
    int64_t n_rank_line_sections_ = 0; // counter 41: sections the _lines calls ranked with a row built from a USER line
    DevBuf<float> rk_items_;           // a _lines call's prepared item side: [num_item][pitch] rows, then [num_item] biases
    int64_t n_item_topn_sections_ = 0; // counter 49: sections listed by svdf_item_topn (its unit rows and zero biases live in rk_items_)
    int64_t n_rank_cand_sections_ = 0; // counter 42: sections the _cand calls ranked over a candidate list
    long rank_cand_form_ = 0;          // knob rank_cand_form: 0 the measured choice, 1 one lane per pair, 2 the staged score kernel
    DevBuf<int> ca_in_, ca_out_;       // a _cand piece's upload (the lists, the tile table) and its results
    DevBuf<float> ca_score_;           // ... and the scores of its pairs
    int64_t n_rank_negs_sections_ = 0; // counter 43: sections ranked against negatives drawn on the device
    DevBuf<int> ng_id_, ng_neg_;       // a sampled piece's cand_id, filled by k_rank_negs_draw, and its neg_out rows where they are asked for
    int64_t n_pair_src_hbm_ = 0;       // counter 44: passes built from a pair source without the pair columns leaving HBM
    int64_t n_pair_src_fallback_ = 0;  // counter 45: passes built from a pair source through dataset_from_pairs on host columns
    std::vector<PairSource *> pair_sources_;   // the live sources of this handle: forgotten (owner = nullptr) when the handle goes
    int64_t n_pair_src_hard_ = 0;      // counter 46: of the passes under 44 / 45, the hard ones (section 6ad)
    long pair_hard_form_ = 0;          // knob pair_hard_form: 0 the measured choice, 1 a lane per candidate, 2 the staged kernel
    int64_t n_pair_src_weighted_ = 0;  // counter 47: of the passes under 44 / 45, those drawn from a weighted source (section 6ae)
    long pair_weight_form_ = 0;        // knob pair_weight_form: 0 the measured choice, 1 the search of the whole cdf, 2 the guided search
    // what every pass refuses, on the host, before any device work (num_cand = 0: the plain pass)
    void pair_source_admit(const PairSource *src, int num_neg, int num_cand);
    // the pass's columns [n * num_neg] filled in HBM by the plain rule (num_cand = 0) or the hard one (user / pos may be nullptr; score only
    // with the hard rule); an entry that exhausted its draws fails the call
    // order (section 6af; nullptr: the source's own order): the rows are taken in the order sigma of this order_seed, and *same_out is the number
    // of adjacent positions that share their user in the order the pass has (src.same without one)
    void pair_source_launch(const PairSource &src, int num_neg, int num_cand, uint64_t seed, unsigned *d_user, unsigned *d_pos, unsigned *d_neg,
                            float *d_score, const uint64_t *order = nullptr, long *same_out = nullptr);
    int64_t n_pair_src_shuffled_ = 0;  // counter 48: of the passes under 44 / 45, the shuffled ones (section 6af)
    int64_t n_kind_[3] = {0, 0, 0};   // launches of k_basicmf / k_general / k_fused
    DeltaRanges delta_ranges();
    friend struct Dataset;
    friend class Ranker;
};

// ISVDRanker (apex_svd.h:160-197) / SVDFeatureRanker (apex_svd_base.h:597-813) on the device, see svdf_ranker.cpp
class Ranker {
  public:
    Ranker(TypeParam mtype, int device);
    ~Ranker();
    void set_param(const char *name, const char *val);
    void load_model(FILE *fi);
    void init_ranker(int num_item_set);
    // process(vector<int>&, Elem) / process(vector<int>&, SVDPlusBlock): results appended to out (up to cap), count returned
    long process(float label, int ng, int nu, int ni, const unsigned *index, const float *value, int *out, long cap);
    // a whole CSR input of the rank task in one call (the loop of svd_feature_infer.cpp:347-375), sections pipelined
    long process_rows(int num_row, const float *row_label, const int *row_ptr, const unsigned *feat_index, const float *feat_value, int *out, long cap);
    long process_block(int nfb, int tag, const unsigned *ifb, const float *vfb, int num_row, const float *row_label, const int *row_ptr,
                       const unsigned *feat_index, const float *feat_value, int *out, long cap);
    int64_t counter(int what) const {
        return what == 0 ? n_sections_ : (what == 1 ? n_host_sorts_ : (what == 2 ? (int64_t)pos_item_.size() : (what == 3 ? n_tiles_ : (what == 4 ? tie_copy_ns_ : (what == 5 ? tie_wait_ns_ : (what == 6 ? event_wait_ns_ : (what == 7 ? flush_ns_ : -1)))))));
    }
  private:
    std::unique_ptr<Engine> eng_;   // owns the model in HBM, the side tables and the kernel parameter block
    int top_k_ = 0, num_item_set_ = 0, num_item_processed_ = 0;
    long items_on_device_ = 0;
    bool init_end_ = false, user_open_ = false;
    HostCSR items_, spec_;
    std::vector<int> spec_idx_, pos_item_;
    std::vector<int> tagged_, dev_tagged_;   // candidates tagged in the open section / in the section the device's tag array reflects
    long n_banned_ = 0;
    // sections in flight (svdf_ranker.cpp): per slot the pinned staging (one upload per section), its device copy, the
    // section's counters / positives' scores / NaN flag / item_score, the pinned readback and the event behind it
    static constexpr int RANK_SLOTS = 8;
    struct RankSlot {
        unsigned *pin = nullptr, *back = nullptr;
        size_t pin_words = 0, back_words = 0;
        DevBuf<unsigned> d_stage, d_flag;
        DevBuf<int> d_cnt;
        DevBuf<float> d_ps, d_score;
        hipEvent_t ev = nullptr;
    };
    struct RankPending { int slot = 0, npos = 0, take = 0; long n = 0; std::vector<int> pos_item, banned;
                         // a tile of sections sharing one scoring pass (svdf_k_rank.hip: k_rank_score_tile): per section its positives / bans
                         int nsec = 0; std::vector<std::vector<int>> tile_pos, tile_ban; std::vector<int> tile_take; long out_stride = 0; };
    struct TileSec { std::vector<unsigned> user_idx; std::vector<float> user_val; std::vector<int> pos_item, banned; int take = 0; };
    std::vector<TileSec> tile_;      // sections staged for the next tile (process_rows, positions mode, no special samples)
    long tile_n_ = 0;                // the candidate count they were staged against
    std::vector<int> tile_prev_ban_; // candidates whose ban bits the previous tile set (cleared by the next tile's opening kernel)
    DevBuf<unsigned> d_banmask_;
    DevBuf<float> d_tu_tile_;
    void flush_tile();
    bool tile_enabled_ = true;
    int64_t n_tiles_ = 0;
    RankSlot slots_[RANK_SLOTS];
    struct RankChunk { std::vector<int> vals; std::future<std::vector<int>> fut; bool pending = false; };   // one section's results
    std::deque<RankPending> pending_;
    std::deque<RankChunk> chunks_;
    void flush_chunks();
    int next_slot_ = 0;
    bool deferred_ = false;
    int *out_ptr_ = nullptr;
    long out_cap_ = 0, out_n_ = 0;
    void slot_reserve_pin(RankSlot &S, size_t words);
    void slot_reserve_back(RankSlot &S, size_t words);
    void enqueue();
    void resolve();
    void drain_quietly();
    std::vector<signed char> tag_;
    std::vector<unsigned> user_idx_;
    std::vector<float> user_val_;
    DevBuf<float> d_ifactors_, d_ift_, d_ibias_, d_tu_, d_fb_, w_label_, w_value_, w_uval_, w_fbval_, s_label_, s_value_;
    DevBuf<int> w_ptr_, s_ptr_, s_idx_;
    DevBuf<unsigned> w_index_, w_fbidx_, s_index_, d_keys_, d_vals_, d_sel_;
    void *sort_tmp_ = nullptr;
    size_t sort_tmp_bytes_ = 0;
    DevBuf<signed char> d_tag_;
    int64_t n_sections_ = 0, n_host_sorts_ = 0;
    std::unique_ptr<struct TieWork> tie_scores(const float *d_src, long n);
    hipStream_t tie_stream_ = nullptr;
    float *tie_pin_ = nullptr;
    size_t tie_pin_floats_ = 0;
    int64_t event_wait_ns_ = 0, flush_ns_ = 0;   // waiting for a slot's event; staging + enqueueing tiles (includes resolving the oldest slot)
    int64_t tie_copy_ns_ = 0, tie_wait_ns_ = 0;   // tied sections: copying their scores out (a stream sync each); waiting for their sorts at the end
    void stage(HostCSR &dst, int ng, int nu, int ni, const unsigned *index, const float *value);
    void check_item_side(int ng, int nu, int ni, const unsigned *index);
    long rank(int *out, long cap);
};

}  // namespace svdf
#endif

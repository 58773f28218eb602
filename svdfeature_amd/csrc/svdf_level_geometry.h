// svdf_level_geometry.h -- the host-only launch choice of the level kernels of the exact pass: for one conflict-free
// level of n instances, which kernel form runs, how many lanes hold a row and how many 16-byte chunks a lane holds, how many row sets a
// wave keeps in flight after folding, the workgroup size, the grid before and after its padding for the XCD remap, and the row-load and
// row-store cache policy in effect.  Plain C++ without a device call: launch_basicmf (svdf_k_basic.hip), launch_fused (svdf_k_fused.hip)
// and launch_fewrow_fast (svdf_k_fewrow.hip) launch what these functions say, the chain queries answer from them, and the test probe
// svdf_level_geometry reports them from a host-only handle (tests/level_geometry.py restates the rule).
#ifndef SVDF_LEVEL_GEOMETRY_H_
#define SVDF_LEVEL_GEOMETRY_H_

#include <algorithm>
#include <cstddef>

#include "svdf_types.h"

namespace svdf {

enum LevelForm {
    LEVEL_BASIC_FAST = 1,      // k_basicmf<LPI, G, true, true, true>: unit values, full rows (k = 4 LPI), the contract configuration
    LEVEL_BASIC_UNIT = 2,      // k_basicmf<LPI, G, true, false, false>: unit values, the general instruction stream
    LEVEL_BASIC_VALUES = 3,    // k_basicmf<LPI, G, false, false, false>: feature values from the schedule
    LEVEL_BASIC_SLOTS8 = 4,    // k_basicmf_slots<8, 2, G>: k = 64, eight lanes per row, two chunks per lane
    LEVEL_BASIC_SLOTS16 = 5,   // k_basicmf_slots<16, 4, G>: k = 256, sixteen lanes per row, four chunks per lane
    LEVEL_FUSED = 6,           // k_fused<LPI, NU, NI, G, FULL>, G = 1 or 2
    LEVEL_FUSED_HOT = 7,       // k_fused<LPI, 2, NI, 1, FULL, true>: 1024 threads, the relaxed shared user row summed in LDS
    LEVEL_FEWROW_FAST = 8,     // k_fewrow_fast<LPI, NU, NI, FULL>
    LEVEL_FEWROW_SLOTS16 = 9,  // k_fewrow_slots<16, 2, NU, NI>: k = 128, sixteen lanes per row, two chunks per lane
};
// the tuning knobs a form reaches: changing a knob whose bit is clear changes nothing in the launch of that form
enum { LEVEL_KNOB_GROUPS = 1, LEVEL_KNOB_BLOCK = 2, LEVEL_KNOB_REMAP = 4, LEVEL_KNOB_LOAD = 8, LEVEL_KNOB_STORE = 16 };

struct LevelShape {
    int form;          // LevelForm
    int lpi;           // the lane class of the row width (lanes_per_instance): the template argument of the lane-group kernels
    int lanes;         // lanes that hold one row
    int chunks;        // 16-byte chunks of a row per lane
    int full;          // the row fills its lanes (k = 4 lanes chunks): no per-lane bounds test
    int groups;        // row sets per wave after folding
    int block;         // threads per workgroup
    int nu, ni;        // user / item slots of the few-row template (0 for the basic forms)
    long per_set;      // instances of one row set: 64 / lanes
    long per_block;    // instances of one workgroup: (block / 64) groups per_set
    long grid_work;    // workgroups that have work: ceil(n / per_block)
    long grid;         // workgroups launched: grid_work, padded to a multiple of 8 under the XCD remap
    int remap;         // the tile permutation (blockIdx & 7) * (grid >> 3) + (blockIdx >> 3) is on
    int load;          // row gathers: 0 plain, 1 nontemporal
    int store;         // row stores: 0 plain, 1 nontemporal, 2 write-through
    int knobs;         // LEVEL_KNOB_* bits of the knobs this launch reads
    size_t lds;        // dynamic LDS bytes (LEVEL_FUSED_HOT only)
};

// lanes of the lane-group kernels for a row of k factors: the power of two that holds its chunks, 64 at most (wide rows: several per lane)
static inline int level_lane_class(int k) {
    const int chunks = (k + 3) / 4;
    int lpi = 1;
    while (lpi < chunks && lpi < 64) lpi <<= 1;
    return lpi;
}
// load_mode knob -> DevParams::load_mode.  2 = auto: nontemporal row gathers for rows of two cache lines or more
static inline int level_load_mode(int knob, int pitch) { return knob == 2 ? (pitch >= 64 ? 1 : 0) : knob; }

// the configuration of the contract workload: linear link, L2 decay by one factor, user bias on, no clamp, no per-range decay
static inline bool level_plain_config(const DevParams &P) {
    return P.active_type == ACT_LINEAR && P.reg_method == 0 && P.no_user_bias == 0 && P.user_nonnegative == 0 && P.u_rng.n == 0 && P.i_rng.n == 0;
}
// ... with unit values under the basic_i8 knob: what k_basicmf_slots is specialised for (its forms need store_mode 0 as well)
static inline bool basicmf_slots_config(const DevParams &P, bool unit) { return P.basic_i8 && unit && level_plain_config(P); }
// runs of narrow levels in one launch (k_basicmf_slots_chain)
static inline bool basicmf_chain_applies(const DevParams &P, bool unit) { return basicmf_slots_config(P, unit) && P.store_mode == 0 && P.k == 64; }
// what k_fewrow_fast is specialised for: no global feature in the data set, no relaxed ids, L2 decay, no per-range decay, no clamp
static inline bool fewrow_fast_config(const DevParams &P, bool has_globals) {
    return !has_globals && !P.relax_global && P.relax_user_from == 0xFFFFFFFFu && P.relax_item_from == 0xFFFFFFFFu &&
           P.reg_method == 0 && P.u_rng.n == 0 && P.i_rng.n == 0 && P.user_nonnegative == 0;
}
static inline bool fewrow_slots16_applies(const DevParams &P, bool has_globals) {
    return P.fewrow_fast && fewrow_fast_config(P, has_globals) && P.k == 128 && P.fewrow_i16 == 1;
}
// runs of narrow levels in one launch (k_fewrow_slots_chain)
static inline bool fewrow_chain_applies(const DevParams &P, bool has_globals) { return fewrow_slots16_applies(P, has_globals); }

// per_block, grid_work, grid, remap of a shape whose lanes, groups and block are set
static inline void level_grid(LevelShape &sh, const DevParams &P, long n) {
    sh.per_set = 64 / sh.lanes;
    sh.per_block = (long)(sh.block / 64) * sh.groups * sh.per_set;
    sh.grid_work = (n + sh.per_block - 1) / sh.per_block;
    sh.remap = P.xcd_remap ? 1 : 0;
    sh.grid = sh.remap ? (sh.grid_work + 7) & ~7L : sh.grid_work;
}

// launch_basicmf: one (user, item) instance per lane group.  groups_per_wave / block_threads: the knobs, 0 = the tuned default
static inline LevelShape basicmf_level_shape(const DevParams &P, bool unit, long n, int groups_per_wave, int block_threads) {
    LevelShape sh = LevelShape();
    const int lpi = level_lane_class(P.k);
    // 0 = tuned default (tools/sweep_knobs.py on MI355X with the FULL/FAST specialisation): k=64 (16 lanes per row) wants
    // 4 row sets in flight per wave in 64-thread blocks (24.9 ms/pass; 26.3 with one row set), k=256 two row sets, every
    // other width one row set per wave in 256-thread blocks
    // (tools/ab_knob.py, in-process A/B: k=64 8 lanes x 2 chunks with 4 row sets 23.6 vs 24.4 ms per 100 M; k=256 16 lanes x 4 chunks with
    // one row set 18.5 vs 20.2 ms per 25 M; k=128 16 lanes x 2 chunks 22.3 vs 22.3 ms per 50 M: no gain, the lane-group kernel stays)
    const bool slots_cfg = basicmf_slots_config(P, unit);
    if (groups_per_wave <= 0) {
        groups_per_wave = lpi == 16 ? 4 : (lpi == 64 ? (slots_cfg && P.k == 256 ? 1 : 2) : 1);
        // k = 64 in the 8-lane layout: 8 instances per row set.  A full-size level (53 K instances) wants 4 row sets per wave (1.6 waves
        // per SIMD: 23.6 ms per pass against 26.6 with 2 and 27.5 with 1), the 17 K-instance levels of one rank's window of an 8-GPU
        // run want 1 (7.66 ms per pass against 8.09 with 2 and 9.10 with 4, tools/shard8_knobs.sh): aim at ~1 800 waves per launch
        if (slots_cfg && P.k == 64) groups_per_wave = (int)std::min<long>(4, std::max<long>(1, (n + 7200) / 14400));
    }
    if (block_threads <= 0) block_threads = lpi == 16 ? 64 : 256;
    const int G = groups_per_wave;
    sh.groups = (G == 1 || G == 2 || G == 3 || G == 5 || G == 6 || G == 8) ? G : 4;   // the instantiated row-set counts
    sh.block = block_threads;
    sh.lpi = lpi;
    // specialised instruction stream for the configuration of the contract workload, general one otherwise
    const bool fast = level_plain_config(P) && P.store_mode == 0;
    sh.lanes = lpi; sh.chunks = 1; sh.full = P.k == 4 * lpi;
    sh.load = P.load_mode & 1; sh.store = 0;
    sh.knobs = LEVEL_KNOB_GROUPS | LEVEL_KNOB_BLOCK | LEVEL_KNOB_REMAP | LEVEL_KNOB_LOAD | LEVEL_KNOB_STORE;
    if (unit && fast && lpi == 16 && P.k == 64 && P.basic_i8) {
        sh.form = LEVEL_BASIC_SLOTS8; sh.lanes = 8; sh.chunks = 2;
    } else if (unit && fast && lpi == 64 && P.k == 256 && P.basic_i8) {
        sh.form = LEVEL_BASIC_SLOTS16; sh.lanes = 16; sh.chunks = 4;
    } else if (unit && fast && sh.full) {
        sh.form = LEVEL_BASIC_FAST;
    } else {
        sh.form = unit ? LEVEL_BASIC_UNIT : LEVEL_BASIC_VALUES;
        sh.store = P.store_mode;
    }
    if (sh.form == LEVEL_BASIC_SLOTS8 || sh.form == LEVEL_BASIC_SLOTS16) {   // the slots forms always gather nontemporal
        sh.load = 1;
        sh.knobs &= ~LEVEL_KNOB_LOAD;
    }
    level_grid(sh, P, n);
    return sh;
}

// launch_fewrow_fast: the few-row step in its usual configuration, one row set per wave
static inline LevelShape fewrow_level_shape(const DevParams &P, int max_nu, int max_ni, long n, int block_threads) {
    LevelShape sh = LevelShape();
    // one-wave workgroups: a level of these workloads is a few hundred to a few thousand waves, and 64-thread blocks spread them over
    // four times as many CUs (tools/ab_knob.py: neighbourhood 87.3 vs 91.8 ms per pass with 256; rank pairs 45.2 vs 45.4: flat)
    if (block_threads <= 0) block_threads = 64;
    sh.lpi = level_lane_class(P.k);
    sh.groups = 1; sh.block = block_threads;
    sh.nu = max_nu <= 1 ? 1 : 2; sh.ni = max_ni <= 1 ? 1 : 2;
    sh.store = 0;
    sh.knobs = LEVEL_KNOB_BLOCK | LEVEL_KNOB_REMAP | LEVEL_KNOB_LOAD;
    // (eight lanes with four chunks each measured slower at k = 128: 46.7 vs 45.2 ms per 50 M pairs; 32 lanes, one chunk: 48.9)
    if (P.k == 128 && P.fewrow_i16 == 1) {
        sh.form = LEVEL_FEWROW_SLOTS16; sh.lanes = 16; sh.chunks = 2; sh.full = 1;
        sh.load = 1;   // always nontemporal
        sh.knobs &= ~LEVEL_KNOB_LOAD;
    } else {
        sh.form = LEVEL_FEWROW_FAST; sh.lanes = sh.lpi; sh.chunks = 1; sh.full = P.k == 4 * sh.lpi;
        sh.load = P.load_mode & 1;
    }
    level_grid(sh, P, n);
    return sh;
}

// launch_fused: few-row instances (<= 2 user ids, <= 2 item ids, any number of globals)
static inline LevelShape fused_level_shape(const DevParams &P, bool has_globals, int max_nu, int max_ni, long n, int groups_per_wave, int block_threads) {
    if (P.fewrow_fast && fewrow_fast_config(P, has_globals)) return fewrow_level_shape(P, max_nu, max_ni, n, block_threads);
    LevelShape sh = LevelShape();
    const int lpi = level_lane_class(P.k);
    if (groups_per_wave <= 0) groups_per_wave = lpi == 16 ? 2 : 1;
    if (block_threads <= 0) block_threads = 64;   // one-wave workgroups, see fewrow_level_shape
    sh.form = LEVEL_FUSED;
    sh.lpi = lpi; sh.lanes = lpi; sh.chunks = 1; sh.full = P.k == 4 * lpi;
    sh.nu = max_nu <= 1 ? 1 : 2; sh.ni = max_ni <= 1 ? 1 : 2;
    sh.block = block_threads;
    sh.load = P.load_mode & 1; sh.store = 0;
    sh.knobs = LEVEL_KNOB_GROUPS | LEVEL_KNOB_BLOCK | LEVEL_KNOB_REMAP | LEVEL_KNOB_LOAD;
    // relaxed shared user feature in the last user slot: big workgroups that pre-reduce its changes in LDS
    const bool hot = sh.nu == 2 && P.relax_user_from != 0xFFFFFFFFu && P.hot_reduce;
    if (hot) {
        sh.form = LEVEL_FUSED_HOT; sh.groups = 1; sh.block = 1024;
        sh.knobs &= ~(LEVEL_KNOB_GROUPS | LEVEL_KNOB_BLOCK);
    } else if (sh.nu + sh.ni <= 3) {
        sh.groups = groups_per_wave >= 2 ? 2 : 1;   // two row sets per wave at most: every value above folds to 2
    } else {
        sh.groups = 1;                              // 2 + 2 slots: one row set (registers)
        sh.knobs &= ~LEVEL_KNOB_GROUPS;
    }
    level_grid(sh, P, n);
    if (hot) sh.lds = (size_t)sh.per_block * ((size_t)lpi * 16 + 8);
    return sh;
}

}  // namespace svdf
#endif

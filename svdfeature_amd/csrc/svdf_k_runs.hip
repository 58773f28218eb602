// svdf_k_runs.hip -- RUNS of an item's consecutive ratings as schedule units (knob "runs_exec").
//
// The contract workload moves 2 factor rows per rating (1072 B at k = 64).  Consecutive ratings of ONE item -- consecutive in
// the item's own file order; they are ~n / count positions apart in the file -- can share the item's row: a lane group reads it once, walks up
// to R ratings with it in registers, writes it once.  A run is a valid unit of a conflict-free schedule when nothing else touches its rows
// "inside" it, and that is a FILE-ORDER fact: rating y (user u) may join the run headed at file position h iff u's previous rating lies
// before h.  Then executing whole runs in the order of their heads is a sequential reordering that keeps every row's touches in file order:
// u's previous rating belongs to a run with an earlier head, u's next rating z can only join a run whose head lies behind y, and the item's
// own ratings are walked in order.  So:
//   1. prev[p] = file position of the previous rating of p's user        (stable radix sort of (user, position), neighbours)
//   2. the item-major list of positions                                   (stable radix sort of (item, position))
//   3. one thread per item walks its list and cuts it into runs           (k_runs_form: head flags, index in run)
//   4. runs numbered by the file position of their head                   (exclusive scan of the head flags)
//   5. the runs' columns (item, R users, R labels; absent users marked)   (k_runs_fill)
//   6. the EXISTING device level scheduler over runs as units with 1 + R row slots (svdf_k_sched.hip), columns gathered into level order
// and a level is one launch of k_basicmf_runs_soa: per rating the arithmetic of k_basicmf_slots in file order inside the run -- the same bits
// as one instance per lane group (tests/test_gpu_runs.py: == the level-by-level pass == the oracle).
// Uniform contract stream, runs of at most 4: 1 874 levels -> ~680, 3.0 - 3.5 ratings per run, the item row's bytes divided by the run length.
#include "svdf_device.h"

namespace svdf {

// ids of both columns against their limits (the reference's messages are raised by the host from the flag word: bit 0 user, bit 1 item)
__global__ __launch_bounds__(256) void k_runs_check(const unsigned *user, const unsigned *item, long n, unsigned nu, unsigned ni, unsigned *flag) {
    const long stride = (long)gridDim.x * blockDim.x;
    unsigned bad = 0u;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (user[p] >= nu) bad |= 1u;
        if (item[p] >= ni) bad |= 2u;
    }
    if (bad) atomicOr(flag, bad);
}
// keys / pos: positions stably sorted by user id: prev[pos[j]] = pos[j - 1] when the users agree, else 0xFFFFFFFF
__global__ __launch_bounds__(256) void k_runs_prev(const unsigned *keys, const unsigned *pos, long n, unsigned *prev) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
        prev[pos[j]] = (j > 0 && keys[j - 1] == keys[j]) ? pos[j - 1] : 0xFFFFFFFFu;
}
// one thread per item: its ratings are ikeys == item in ipos (ascending file positions).  head[p] = 1 at the first rating of a run,
// head_of[p] = the head's position, idx[p] = the rating's index inside its run
__global__ __launch_bounds__(256) void k_runs_form(const unsigned *ikeys, const unsigned *ipos, long n, unsigned num_item, const unsigned *prev, int R,
                                                   unsigned *head, unsigned *head_of, unsigned char *idx) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < (long)num_item; it += stride) {
        long lo = 0, hi = n;   // first j with ikeys[j] >= it
        while (lo < hi) { const long mid = (lo + hi) >> 1; if (ikeys[mid] < (unsigned)it) lo = mid + 1; else hi = mid; }
        unsigned h = 0u;
        int len = 0;
        for (long j = lo; j < n && ikeys[j] == (unsigned)it; j++) {
            const unsigned p = ipos[j];
            const unsigned pv = prev[p];
            // (the user's previous rating must lie before the head; a rating of the same user INSIDE the run -- the item rated twice in a row --
            // has prev >= h and starts a new run)
            if (len > 0 && len < R && (pv == 0xFFFFFFFFu || pv < h)) {
                head[p] = 0u; head_of[p] = h; idx[p] = (unsigned char)len;
                len++;
            } else {
                head[p] = 1u; head_of[p] = p; idx[p] = 0;
                h = p; len = 1;
            }
        }
    }
}
// unit_at[p] = exclusive scan of head[] (valid at heads).  Every rating writes itself into slot idx[p] of its run's columns.
__global__ __launch_bounds__(256) void k_runs_fill(const unsigned *user, const unsigned *item, const float *label, long n, const unsigned *unit_at,
                                                   const unsigned *head_of, const unsigned char *idx, long nunit, unsigned *c_item, unsigned *c_user, float *c_label) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const unsigned un = unit_at[head_of[p]];
        const int j = idx[p];
        c_user[(size_t)j * (size_t)nunit + un] = user[p];
        c_label[(size_t)j * (size_t)nunit + un] = label[p];
        if (j == 0) c_item[un] = item[p];
    }
}
__global__ __launch_bounds__(256) void k_runs_fill_u32(unsigned *v, long n, unsigned x) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) v[j] = x;
}
static inline int runs_grid(long n) { long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g)); }
void launch_runs_check(const unsigned *user, const unsigned *item, long n, unsigned nu, unsigned ni, unsigned *flag, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs_check, dim3(runs_grid(n)), dim3(256), 0, st, user, item, n, nu, ni, flag);
}
void launch_runs_prev(const unsigned *keys, const unsigned *pos, long n, unsigned *prev, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs_prev, dim3(runs_grid(n)), dim3(256), 0, st, keys, pos, n, prev);
}
void launch_runs_form(const unsigned *ikeys, const unsigned *ipos, long n, unsigned num_item, const unsigned *prev, int R, unsigned *head, unsigned *head_of,
                      unsigned char *idx, hipStream_t st) {
    if (n > 0 && num_item > 0) hipLaunchKernelGGL(k_runs_form, dim3(runs_grid((long)num_item)), dim3(256), 0, st, ikeys, ipos, n, num_item, prev, R, head, head_of, idx);
}
void launch_runs_fill(const unsigned *user, const unsigned *item, const float *label, long n, const unsigned *unit_at, const unsigned *head_of,
                      const unsigned char *idx, long nunit, unsigned *c_item, unsigned *c_user, float *c_label, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs_fill, dim3(runs_grid(n)), dim3(256), 0, st, user, item, label, n, unit_at, head_of, idx, nunit, c_item, c_user, c_label);
}
__global__ __launch_bounds__(256) void k_runs_iota(unsigned *v, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) v[j] = (unsigned)j;
}
void launch_runs_iota(unsigned *v, long n, hipStream_t st) {
    if (n <= 0) return;
    long grid = (n + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(k_runs_iota, dim3((int)grid), dim3(256), 0, st, v, n);
}
void launch_runs_fill_u32(unsigned *v, long n, unsigned x, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_runs_fill_u32, dim3(runs_grid(n)), dim3(256), 0, st, v, n, x);
}

// ------------------------------------------------------------------------------------------------- order inside a level (knob "runs_order")
// A wave carries 64 / LANES runs and walks as many steps -- and gather rounds -- as its longest one, so a level's runs are sorted by length, longest first,
// item order inside a length: the units of a level commute, and the in-level order is a free sort key of the scheduler (profiles/r28_runs_order.md).
// A run's ratings fill its user slots from 0 without holes: its length is its last present slot + 1.
__device__ __forceinline__ int runs_length(const RunSchedule &S, size_t at, int R) {
    int len = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (j < R && S.user[j][at] != (unsigned)SLOT_ABSENT) len = j + 1;
    return len;
}
__global__ __launch_bounds__(256) void k_runs_order_key(const unsigned *c_item, const unsigned *c_user, long nunit, int R, unsigned num_item, unsigned *key) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long un = (long)blockIdx.x * blockDim.x + threadIdx.x; un < nunit; un += stride) {
        int len = 0;
        for (int j = 0; j < R; j++)
            if (c_user[(size_t)j * (size_t)nunit + (size_t)un] != (unsigned)SLOT_ABSENT) len = j + 1;
        key[un] = (unsigned)(R - len) * num_item + c_item[un];
    }
}
// With xcd_remap the pass kernel gives each of the 8 XCDs one contiguous eighth of a level, and a level sorted by length alone leaves the long runs to the
// first XCDs (measured: +9 % per pass).  So the level's full row sets are dealt round robin into 8 contiguous shares: share x = the sets x, x + 8, ... of
// the sorted order, each share sorted by length again.  Sets stay whole and aligned to the level's begin; the last, partial set stays last.
__global__ __launch_bounds__(256) void k_runs_order_deal(const int *order, int *out, const long *level_ptr, int nlev, long nunit, int ips) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nunit; s += stride) {
        int lo = 0, hi = nlev - 1;   // the last level that begins at or before s
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (level_ptr[mid] <= s) lo = mid; else hi = mid - 1; }
        const long begin = level_ptr[lo], nf = (level_ptr[lo + 1] - begin) / ips, p = s - begin;
        long to = s;
        if (p < nf * ips) {
            const long q = p / ips;
            const int x = (int)(q & 7);
            long base = 0;
            for (int y = 0; y < x; y++) base += (nf - y + 7) / 8;   // the sets q' < nf with q' % 8 == y
            to = begin + (base + (q >> 3)) * ips + p % ips;
        }
        out[to] = order[s];
    }
}
void launch_runs_order_deal(const int *order, int *out, const long *level_ptr, int nlev, long nunit, int ips, hipStream_t st) {
    if (nunit > 0 && nlev > 0) hipLaunchKernelGGL(k_runs_order_deal, dim3(runs_grid(nunit)), dim3(256), 0, st, order, out, level_ptr, nlev, nunit, ips);
}
// Over the level-sorted columns, once per data set.  The aligned sets of `ips` runs from each level's begin are the rows one wave of k_basicmf_runs_soa
// carries: tot[0] += the set's longest run (the steps that wave walks), tot[1] += 1 for a set whose runs differ in length; tot[1 + length] += the runs of
// that length.
__global__ __launch_bounds__(256) void k_runs_order_stats(const RunSchedule S, const long *level_ptr, int nlev, long nunit, int R, int ips, unsigned long long *tot) {
    const long stride = (long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    unsigned long long steps = 0ull, mixed = 0ull, cnt[8];
#pragma unroll
    for (int c = 0; c < 8; c++) cnt[c] = 0ull;
    for (long base = (long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < nunit; base += stride) {   // a wave-uniform bound: ballots below
        const long s = base + lane;
        const bool on = s < nunit;
        int len = 0;
        if (on) {
            int lo = 0, hi = nlev - 1;   // the last level that begins at or before s
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (level_ptr[mid] <= s) lo = mid; else hi = mid - 1; }
            len = runs_length(S, (size_t)s, R);
            const long begin = level_ptr[lo], end = level_ptr[lo + 1];
            if ((s - begin) % ips == 0) {
                int mx = len;
                bool mix = false;
                for (int t = 1; t < ips && s + t < end; t++) {
                    const int l2 = runs_length(S, (size_t)(s + t), R);
                    mix = mix || l2 != len;
                    mx = l2 > mx ? l2 : mx;
                }
                steps += (unsigned long long)mx;
                mixed += mix ? 1ull : 0ull;
            }
        }
#pragma unroll
        for (int c = 1; c < 8; c++) cnt[c] += (unsigned long long)__popcll(__ballot(on && len == c));   // the same sums in every lane
    }
    for (int o = 32; o > 0; o >>= 1) { steps += __shfl_xor(steps, o); mixed += __shfl_xor(mixed, o); }
    if (lane == 0) {
        if (steps) atomicAdd(tot, steps);
        if (mixed) atomicAdd(tot + 1, mixed);
#pragma unroll
        for (int c = 1; c < 8; c++)
            if (cnt[c]) atomicAdd(tot + 1 + c, cnt[c]);
    }
}
void launch_runs_order_key(const unsigned *c_item, const unsigned *c_user, long nunit, int R, unsigned num_item, unsigned *key, hipStream_t st) {
    if (nunit > 0) hipLaunchKernelGGL(k_runs_order_key, dim3(runs_grid(nunit)), dim3(256), 0, st, c_item, c_user, nunit, R, num_item, key);
}
void launch_runs_order_stats(const RunSchedule &S, const long *level_ptr, int nlev, long nunit, int R, int ips, unsigned long long *tot, hipStream_t st) {
    if (nunit > 0 && nlev > 0) hipLaunchKernelGGL(k_runs_order_stats, dim3(runs_grid(nunit)), dim3(256), 0, st, S, level_ptr, nlev, nunit, R, ips, tot);
}

// ------------------------------------------------------------------------------------------------- operand staging (knob "runs_stage")
// Every row is read and written at every touch anyway, so the write can go where the row's NEXT reader will look: slot s * (1 + R) + j of the
// staging buffers, s = the reader's position in level order, j = 0 its item row, 1 .. R its users' rows.  The slot NUMBER is run-major, and so are the
// words kept per slot (dst, bias; the labels beside them): what the runs of one wave need of each is one contiguous block.  The slot's ROW lies
// plane-major, row j * nunit + s of stage_row (runs_row_of): rows laid out run-major cost 1.2 ms per pass (profiles/r37_runs_pack.md).  The links are a
// file-order fact too: runs
// are numbered by head position and a row's touches ascend in that number, so a stable sort of (row, unit number) puts every touch next to its successor.
// pos_of[order[s]] = s: unit number -> position in level order
__global__ __launch_bounds__(256) void k_runs_inverse(const int *order, long nunit, unsigned *pos_of) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < nunit; s += stride) pos_of[order[s]] = (unsigned)s;
}
// the operands in unit-number order: entry un * (1 + R) + j = (row id in the scheduler's numbering: users first, then items; slot).  Holes get the key
// 0xFFFFFFFF and sort behind every row.
__global__ __launch_bounds__(256) void k_runs_operands(const RunSchedule S, const unsigned *pos_of, long nunit, int R, unsigned num_user, unsigned *keys, unsigned *vals) {
    const long stride = (long)gridDim.x * blockDim.x, m = nunit * (1 + R);
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
        const long un = t / (1 + R);
        const int j = (int)(t - un * (1 + R));
        const unsigned s = pos_of[un];
        const unsigned id = j == 0 ? num_user + S.item[s] : S.user[j - 1][s];
        keys[t] = (j > 0 && id == (unsigned)SLOT_ABSENT) ? 0xFFFFFFFFu : id;
        vals[t] = (unsigned)((long)s * (1 + R) + j);
    }
}
// the labels run-major, next to the slots: out[s * R + j] = label[j][s] of the level-sorted planes (the planes stay: the pass on rows in W reads them)
__global__ __launch_bounds__(256) void k_runs_label_rm(const RunSchedule S, long nunit, int R, float *out) {
    const long stride = (long)gridDim.x * blockDim.x, m = nunit * R;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
        const long s = t / R;
        out[t] = S.label[(int)(t - s * R)][s];
    }
}
void launch_runs_label_rm(const RunSchedule &S, long nunit, int R, float *out, hipStream_t st) {
    if (nunit > 0) hipLaunchKernelGGL(k_runs_label_rm, dim3(runs_grid(nunit * R)), dim3(256), 0, st, S, nunit, R, out);
}
// keys / vals sorted: dst of every slot, and the slot of every touched row's first touch
__global__ __launch_bounds__(256) void k_runs_links(const unsigned *keys, const unsigned *vals, long m, unsigned row0, unsigned *dst, unsigned *first) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += stride) {
        const unsigned key = keys[t], slot = vals[t];
        if (key == 0xFFFFFFFFu) { dst[slot] = (unsigned)SLOT_ABSENT; continue; }
        dst[slot] = (t + 1 < m && keys[t + 1] == key) ? vals[t + 1] : ((unsigned)RUNS_HOME | (row0 + key));
        if (t == 0 || keys[t - 1] != key) first[key] = slot;
    }
}
void launch_runs_stage_links(const RunSchedule &S, const int *order, long nunit, int R, unsigned num_user, unsigned row0, unsigned *pos_of, unsigned *ka, unsigned *kb,
                             unsigned *va, unsigned *vb, void **tmp, size_t *tmp_bytes, unsigned *dst, unsigned *first, long nrow, hipStream_t st) {
    if (nunit <= 0) return;
    const long m = nunit * (1 + R);
    hipLaunchKernelGGL(k_runs_inverse, dim3(runs_grid(nunit)), dim3(256), 0, st, order, nunit, pos_of);
    hipLaunchKernelGGL(k_runs_operands, dim3(runs_grid(m)), dim3(256), 0, st, S, pos_of, nunit, R, num_user, ka, va);
    device_sort_pairs_u32(ka, kb, va, vb, m, tmp, tmp_bytes, st);
    launch_runs_fill_u32(first, nrow, (unsigned)SLOT_ABSENT, st);
    hipLaunchKernelGGL(k_runs_links, dim3(runs_grid(m)), dim3(256), 0, st, kb, vb, m, row0, dst, first);
}
// Before level 0 of a staged pass: W is the truth between passes, so every touched row (and its bias) is copied into the slot of its first touch.
// first[r], r in the scheduler's numbering = W row row0 + r; LPR lanes per row
// (ns = 1 + R slots per run.)  Where the ROW of slot d = s * ns + j lies in stage_row: plane-major, row j * nunit + s
__device__ __forceinline__ size_t runs_row_of(unsigned d, int ns, size_t nunit) {
    const unsigned s = d / (unsigned)ns;
    return (size_t)(d - s * (unsigned)ns) * nunit + (size_t)s;
}
template <int LPR>
__global__ __launch_bounds__(256) void k_runs_stage_in(const DevParams P, const unsigned *first, long nrow, unsigned row0, float *stage_row, float *stage_bias, int ns, long nunit) {
    const int L = threadIdx.x % LPR;
    const long per = 256 / LPR, stride = (long)gridDim.x * per;
    for (long r = (long)blockIdx.x * per + threadIdx.x / LPR; r < nrow; r += stride) {
        const unsigned slot = first[r];
        if (slot == (unsigned)SLOT_ABSENT) continue;
        store_row<LPR>(stage_row, runs_row_of(slot, ns, (size_t)nunit), P.pitch, L, P.k, load_row_nt<LPR>(P.W, (size_t)row0 + (size_t)r, P.pitch, L, P.k));
        if (L == 0) stage_bias[slot] = P.bias[(size_t)row0 + (size_t)r];
    }
}
void launch_runs_stage_in(const DevParams &P, const unsigned *first, long nrow, unsigned row0, float *stage_row, float *stage_bias, int ns, long nunit, hipStream_t st) {
    if (nrow <= 0) return;
    const long per = P.k == 128 ? 8 : 16;
    long grid = (nrow + per - 1) / per;
    if (grid > 16384) grid = 16384;
    if (P.k == 128) hipLaunchKernelGGL(k_runs_stage_in<32>, dim3((int)grid), dim3(256), 0, st, P, first, nrow, row0, stage_row, stage_bias, ns, nunit);
    else hipLaunchKernelGGL(k_runs_stage_in<16>, dim3((int)grid), dim3(256), 0, st, P, first, nrow, row0, stage_row, stage_bias, ns, nunit);
}

// ------------------------------------------------------------------------------------------------- the pass
// One level of runs.  S.item[s], S.user[j][s], S.label[j][s] (j < R; S.user[j][s] == SLOT_ABSENT: the run has fewer than j + 1 ratings).
// STAGED (knob "runs_stage"): the run's rows and biases are read from its own staging slots -- addresses that are arithmetic on s, no id has to arrive
// first -- and written to the slots of their next readers (S.dst), home to W / P.bias at a row's last touch of the pass.  The steps are the same lines.
__device__ __forceinline__ unsigned load_u32_nt(const unsigned *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ float load_f32_nt(const float *p) { return __builtin_nontemporal_load(p); }
// Store policy of the STAGED form (knob "runs_store", profiles/r39_runs_store.md).  A staged launch writes every row to a line nobody has read -- its next
// reader's slot -- and a plain store leaves that line dirty in the XCD's L2 until the kernel ends: up to an L2's worth of write-back that nothing overlaps.
// SP is the knob's value.  The rows (whole 128-byte lines) and the 4-byte bias words do not want the same policy, and the knob names the best measured
// combination of each kind: 0 = all plain; 1 = the bias words nontemporal, the rows plain (nontemporal rows are slower than plain ones with every kind
// of bias store); 2 = rows and bias words sc1 write-through (sc1 rows with plain or nontemporal bias words lose to 0).  A row's store is one instruction
// whether it goes to a slot or home to W (the target is chosen per lane): a policy of their own for the home rows costs a divergent branch and lost.
// (a row of the STAGED form: L < K / 4 always, K = 4 * LANES * V, so no lane is masked)
template <int SP>
__device__ __forceinline__ void runs_store_row(float *W, size_t row, int pitch, int L, const float4 v) {
    float *ptr = W + row * (size_t)pitch + (size_t)L * 4;
    if constexpr (SP != 2) {
        *reinterpret_cast<float4 *>(ptr) = v;
    } else {
        // (the s_nop 1: on gfx950 a store of more than 64 bits needs two wait states before a VALU instruction overwrites its data registers.  The compiler
        // keeps that distance behind its own stores but does not look inside an asm statement, and it does place such a write right behind this one.)
        svdf_f4 x = {v.x, v.y, v.z, v.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(ptr), "v"(x) : "memory");
    }
}
template <int SP>
__device__ __forceinline__ void runs_store_bias(float *ptr, float x) {
    if constexpr (SP == 0) *ptr = x;
    else if constexpr (SP == 1) __builtin_nontemporal_store(x, ptr);
    else asm volatile("global_store_dword %0, %1, off sc1" ::"v"(ptr), "v"(x) : "memory");
}
#ifdef SVDF_RUNS_STAMPS   // timing build only (never set by the Makefile): wall_clock64() stamps of lane 0 of every wave, 8 per wave, ordinary vector stores
#define RUNS_STAMP(i_) do { if (S.stamps && lane == 0) S.stamps[((size_t)S.stamp_wave0 + (size_t)wave) * 8 + (i_)] = wall_clock64(); } while (0)
#else
#define RUNS_STAMP(i_) do { } while (0)
#endif
// SP: the store policy, the value of the knob "runs_store" (STAGED only)
template <int LANES, int V, int R, int G, bool STAGED, int SP = 0>
__global__ __launch_bounds__(256) void k_basicmf_runs_soa(const DevParams P, const RunSchedule S, long begin, long end) {
    static_assert(STAGED || SP == 0, "the form on rows in W stores plainly");
    constexpr int T = 16 / LANES;
    constexpr int IPS = 64 / LANES;    // runs per wave and row set
    constexpr int K = 4 * LANES * V;
    const int lane = threadIdx.x & 63;
    long tile = blockIdx.x;
    if (P.xcd_remap) tile = (long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const long wave = tile * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int m = (lane & 15) / T;
    const int gslot = (lane >> 4) * T + (lane & (T - 1));
    const int pitch = P.pitch;
    const float dec_u1 = snap_to_one(1.0f - P.lr * P.wd_user), dec_i1 = snap_to_one(1.0f - P.lr * P.wd_item);
    RUNS_STAMP(0);
#pragma unroll 1
    for (int g = 0; g < G; g++) {
        const long w0 = begin + (wave * G + g) * IPS;
        if (w0 >= end) return;
        const long s = w0 + gslot;
        const bool live = s < end;
        const long sc = live ? s : w0;
        unsigned ir, ur[R];   // the rows in W; STAGED: the dst words of the item operand and of the user operands (where each is written)
        float label[R], bu[R], bi;
        float4 p[R][V], q[V];
        int n = 0;
        if constexpr (!STAGED) {
            ir = P.item_off + S.item[sc];
#pragma unroll
            for (int j = 0; j < R; j++) {
                const unsigned u = S.user[j][sc];
                label[j] = S.label[j][sc];
                const bool on = live && u != (unsigned)SLOT_ABSENT;
                ur[j] = P.user_off + (on ? u : 0u);
                if (on) n = j + 1;
            }
#pragma unroll
            for (int v = 0; v < V; v++) q[v] = live ? load_row_nt<K / 4>(P.W, ir, pitch, m + v * LANES, K) : f4zero();
            bi = live ? P.bias[ir] : 0.0f;
#pragma unroll
            for (int j = 0; j < R; j++) {
#pragma unroll
                for (int v = 0; v < V; v++) p[j][v] = f4zero();
                bu[j] = 0.0f;
                if (j < n) {
#pragma unroll
                    for (int v = 0; v < V; v++) p[j][v] = load_row_nt<K / 4>(P.W, ur[j], pitch, m + v * LANES, K);
                    bu[j] = P.bias[ur[j]];
                }
            }
        } else {
            // Slots are numbered run-major, s * (1 + R) + j: the dst words, the biases and the labels of the row set's runs are one block each -- IPS * (1 + R)
            // / IPS * R dwords from the set's first run on, at most one per lane -- and one load instruction each; a lane past the block, or past the
            // level's end in a partial set, loads nothing.  Every lane group takes its run's words out of the blocks with ds_bpermute (a dead group: run w0's,
            // never used).  As planes of their own these columns were 14 of the wave's 24 load instructions, 32 bytes each (profiles/r37_runs_pack.md).
            // The rows themselves stay plane-major, row j * nunit + s of stage_row: one load instruction of the wave reads 8 neighbouring rows, as before.
            constexpr int NS = 1 + R;
            static_assert(IPS * NS <= 64, "a row set's slot words must fit one dword per lane");
            const int nrun = end - w0 < (long)IPS ? (int)(end - w0) : IPS;
            const size_t blk = (size_t)w0 * NS, nun = (size_t)S.nunit, at0 = (size_t)sc;
            unsigned dw = (unsigned)SLOT_ABSENT;
            float lw = 0.0f, bw = 0.0f;
            if (lane < nrun * NS) dw = load_u32_nt(S.dst + blk + lane);
            if (lane < nrun * R) lw = S.label_rm[(size_t)w0 * R + lane];
            if (lane < nrun * NS) bw = load_f32_nt(S.stage_bias + blk + lane);
#pragma unroll
            for (int v = 0; v < V; v++) q[v] = live ? load_row_nt<K / 4>(S.stage_row, at0, pitch, m + v * LANES, K) : f4zero();
            const int g0 = (int)(sc - w0);
#ifdef SVDF_RUNS_STAMPS
            asm volatile("" :: "v"(q[0].x), "v"(q[V - 1].x), "v"(dw), "v"(lw), "v"(bw));
            RUNS_STAMP(1);
#endif
            ir = __shfl(dw, g0 * NS);
#pragma unroll
            for (int j = 0; j < R; j++) ur[j] = __shfl(dw, g0 * NS + 1 + j);
            // One operand per `if (j < n)`, the shape of the loads from W above, but two rows in flight: row j - 1 is waited for after row j has left
            // (14.57 against 14.82 ms per pass with one row in flight, profiles/r37_runs_pack.md section 3; again in profiles/r39_runs_store.md).  The
            // addresses need no id, so the whole read could leave with the dst words -- built and measured: 19.8 against 16.9 ms per pass (W) and 16.2
            // (one row in flight), profiles/r26_runs_stage.md; all user rows at once behind the item row: 15.4 (r37).  The waits are the compiler's,
            // placed in front of an empty statement that reads the row's registers: without one it sends all rows at once.
#pragma unroll
            for (int j = 0; j < R; j++)
                if (live && ur[j] != (unsigned)SLOT_ABSENT) n = j + 1;
#pragma unroll
            for (int j = 0; j < R; j++) {
#pragma unroll
                for (int v = 0; v < V; v++) p[j][v] = f4zero();
                if (j < n) {
#pragma unroll
                    for (int v = 0; v < V; v++) p[j][v] = load_row_nt<K / 4>(S.stage_row, (size_t)(1 + j) * nun + at0, pitch, m + v * LANES, K);
                    if (j > 0) { asm volatile("" :: "v"(p[j - 1][0].x), "v"(p[j - 1][V - 1].x)); if (j < 4) RUNS_STAMP(1 + j); }
                }
            }
            // (the bias and label blocks left before the rows and are here before them: these moves add no memory wait)
            const float b0 = __shfl(bw, g0 * NS);
            bi = live ? b0 : 0.0f;
#pragma unroll
            for (int j = 0; j < R; j++) {
                const float b = __shfl(bw, g0 * NS + 1 + j);
                bu[j] = j < n ? b : 0.0f;
                label[j] = __shfl(lw, g0 * R + j);
            }
        }
        // Every row is here before step 0 (an empty statement that reads a register of each: the compiler places its counted waits in front of
        // it).  Without it the stores below, each under `act`, leave the compiler unsure of what is in flight where the paths meet, and steps
        // 1 ... begin with vmcnt(1) / vmcnt(0): every step waited for the previous step's stores to be acknowledged.  With it the step loop
        // holds no memory wait at all.  (Issuing all R rows at once, without the `if (j < n)` above, was measured too: 20.2 against 17.1 ms per
        // pass, profiles/r13_runs_gather.md -- the row-by-row gather stays.)
#pragma unroll
        for (int j = 0; j < R; j++) asm volatile("" :: "v"(p[j][0].x), "v"(p[j][V - 1].x), "v"(bu[j]));
        RUNS_STAMP(5);
#pragma unroll
        for (int j = 0; j < R; j++) {
            if (!__any(j < n)) break;   // the wave walks as many steps as its longest run (dot_slots is a wave-wide operation)
            // the arithmetic of k_basicmf_slots (= basicmf_wave<K / 4, ., true, true, true>) on (user row j, the item row as the run has left it)
            double bs = 0.0;
            bs += (double)(1.0f * bu[j]); bs += 0.0;
            bs += 0.0;
            bs += (double)(1.0f * bi);
            double sum = (double)P.base_score + bs;
            float4 tu[V], ti[V];
#pragma unroll
            for (int v = 0; v < V; v++) { tu[v] = f4zero(); ti[v] = f4zero(); axpy4(tu[v], p[j][v], 1.0f); axpy4(ti[v], q[v], 1.0f); }
            sum += (double)dot_slots<LANES, V>(tu, ti, m, lane);
            const float pred = (float)sum;
            const float err = (label[j] - pred) * 1.0f;
            const float su = P.lr * err * 1.0f;
            const float si = P.lr * err * 1.0f;
            float nbu = bu[j] + su, nbi = bi + si;
            nbu = nbu * (1.0f - P.lr * P.wd_user_bias);
            nbi = nbi * (1.0f - P.lr * P.wd_item_bias);
            const bool act = j < n;
            float *wb = P.W, *bb = P.bias;
            size_t wr = ur[j], wrow = ur[j];
            if constexpr (STAGED) {   // the row's next reader's slot, or home at its last touch of the pass
                const bool home = (ur[j] & (unsigned)RUNS_HOME) != 0u;
                wb = home ? P.W : S.stage_row; bb = home ? P.bias : S.stage_bias;
                wr = ur[j] & ~(unsigned)RUNS_HOME;
                wrow = home ? wr : runs_row_of((unsigned)wr, 1 + R, (size_t)S.nunit);
            }
#pragma unroll
            for (int v = 0; v < V; v++) {
                float4 wu = p[j][v], wi = q[v];
                axpy4(wu, ti[v], su);
                axpy4(wi, tu[v], si);
                wu.x = wu.x * dec_u1; wu.y = wu.y * dec_u1; wu.z = wu.z * dec_u1; wu.w = wu.w * dec_u1;
                wi.x = wi.x * dec_i1; wi.y = wi.y * dec_i1; wi.z = wi.z * dec_i1; wi.w = wi.w * dec_i1;
                if (act) {
                    if constexpr (STAGED) runs_store_row<SP>(wb, wrow, pitch, m + v * LANES, wu);
                    else store_row<K / 4>(wb, wrow, pitch, m + v * LANES, K, wu);
                    q[v] = wi;
                }
            }
            if (act) {
                if constexpr (STAGED) runs_store_bias<SP>(bb + wr, nbu);
                else bb[wr] = nbu;
                bi = nbi;
            }
        }
        if (live) {
            float *wb = P.W, *bb = P.bias;
            size_t wr = ir, wrow = ir;
            if constexpr (STAGED) {
                const bool home = (ir & (unsigned)RUNS_HOME) != 0u;
                wb = home ? P.W : S.stage_row; bb = home ? P.bias : S.stage_bias;
                wr = ir & ~(unsigned)RUNS_HOME;
                wrow = home ? wr : runs_row_of((unsigned)wr, 1 + R, (size_t)S.nunit);
            }
#pragma unroll
            for (int v = 0; v < V; v++) {
                if constexpr (STAGED) runs_store_row<SP>(wb, wrow, pitch, m + v * LANES, q[v]);
                else store_row<K / 4>(wb, wrow, pitch, m + v * LANES, K, q[v]);
            }
            if constexpr (STAGED) runs_store_bias<SP>(bb + wr, bi);
            else bb[wr] = bi;
        }
        RUNS_STAMP(6);
    }
}
#undef RUNS_STAMP
bool basicmf_runs_soa_applies(const DevParams &P) {
    return P.basic_i8 && P.active_type == ACT_LINEAR && P.reg_method == 0 && P.no_user_bias == 0 && P.user_nonnegative == 0 && P.u_rng.n == 0 && P.i_rng.n == 0 &&
           P.store_mode == 0 && (P.k == 64 || P.k == 128);
}
// k = 64: 8 lanes x 2 chunks per row, 8 runs per wave and row set; k = 128: 16 lanes x 2 chunks, 4 runs
void launch_basicmf_runs_soa(const DevParams &P, const RunSchedule &S, long begin, long end, int R, int G, int block_threads, hipStream_t st) {
    if (end <= begin) return;
    if (G < 1) G = 1;
    if (block_threads != 64 && block_threads != 128 && block_threads != 256) block_threads = 64;
    const int per_wave = P.k == 128 ? 4 : 8;
    const long per_block = (long)(block_threads / 64) * G * per_wave;
    int grid = (int)((end - begin + per_block - 1) / per_block);
    if (P.xcd_remap) grid = (grid + 7) & ~7;
#define RUNS_STAGED(L_, R_, G_, SP_) hipLaunchKernelGGL((k_basicmf_runs_soa<L_, 2, R_, G_, true, SP_>), dim3(grid), dim3(block_threads), 0, st, P, S, begin, end)
#define RUNS_LAUNCH(L_, R_, G_)                                                                                                                          \
    do {                                                                                                                                                \
        if (!S.dst) hipLaunchKernelGGL((k_basicmf_runs_soa<L_, 2, R_, G_, false>), dim3(grid), dim3(block_threads), 0, st, P, S, begin, end);            \
        else if (S.store == 1) RUNS_STAGED(L_, R_, G_, 1);                                                                                              \
        else if (S.store == 2) RUNS_STAGED(L_, R_, G_, 2);                                                                                              \
        else RUNS_STAGED(L_, R_, G_, 0);                                                                                                                \
    } while (0)
#define RUNS_BY_R(L_)                                                                                                          \
    if (R == 2) { if (G >= 2) RUNS_LAUNCH(L_, 2, 2); else RUNS_LAUNCH(L_, 2, 1); }      /* R = user / label columns of the schedule: 2, 4 or 7 */ \
    else if (R == 4) { if (G >= 2) RUNS_LAUNCH(L_, 4, 2); else RUNS_LAUNCH(L_, 4, 1); }                                       \
    else { if (G >= 2) RUNS_LAUNCH(L_, 7, 2); else RUNS_LAUNCH(L_, 7, 1); }
    if (P.k == 128) { RUNS_BY_R(16) } else { RUNS_BY_R(8) }
#undef RUNS_STAGED
#undef RUNS_BY_R
#undef RUNS_LAUNCH
}

}  // namespace svdf

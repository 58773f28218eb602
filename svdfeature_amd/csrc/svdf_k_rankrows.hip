// svdf_k_rankrows.hip -- the effective user rows of the batch ranking calls on a user-group (SVD++) trainer.
//
// The ranker scores a user-group section with tmp_ufactor = tmp_ufeedback + W_user[u] * 1, where tmp_ufeedback = 0 + sum_j W_ufeedback[fid_j]
// * val_j in list order (apex_svd_base.h:719-735, 798-808): k_rank_feedback followed by k_rank_user (svdf_k_rank.hip), one section per
// launch.  k_rank_live_rows forms that row for every section of a piece in one launch, with those kernels' operations -- axpy4: unfused
// multiply, then add, per element a serial fp32 chain in list order -- and writes it to a workspace [nsec][pitch] that the sweeps of
// svdf_k_rankeval.hip / svdf_k_ranktopn.hip read in place of W_user rows.  One lane group (LPI lanes, one float4 each; a whole wave with
// 2 .. 4 float4 per lane for wide rows) owns a section, 64 / LPI sections share a wave.  A list's chain is serial by contract, so a list
// is never split over waves: a long list costs its length.  The row loads of a list do not depend on each other: RR_NB rows are requested
// together ahead of their adds.  Plain vector loads and stores; no LDS, no atomics.
//
// Section 6z adds the rows of sections that bring a USER line (several ids, any value, feature_user children) and, for trainers with a
// feature_item table, k_rank_live_items: the prepared item matrix and bias vector the sweeps read in place of W_item / i_bias.
#include <algorithm>

#include "svdf_device.h"

namespace svdf {

constexpr int RR_NB = 8;   // feedback rows requested at a time (8 x 16 floats per lane for the widest rows: no scratch)

// A NaN VALUE is the one input on which the batch call leaves the ranker: the reference's scalar_map takes a NaN scalar for 1 (its
// |s - 1| > 1e-6 test is false, svdf_device.h: scalar_is_one), so the ranker would add the row unscaled and say nothing.  Here the NaN
// reaches every element of the section's row -- f + NaN -- and flags the section like any NaN score.
__device__ __forceinline__ void rr_poison(float4 &f, float nan) { f.x = f.x + nan; f.y = f.y + nan; f.z = f.z + nan; f.w = f.w + nan; }
template <int V> __device__ __forceinline__ void rr_poison(WideRow<V> &f, float nan) {
#pragma unroll
    for (int v = 0; v < V; v++) rr_poison(f.v[v], nan);
}

// the children of one USER-line id, rows [c0, c1) of the feature_user table in table order: tu += W_user[cid] * cval, RR_NB row loads
// requested ahead of their adds (k_rank_user's inner loop, svdf_k_rank.hip)
template <int LPI, typename R>
__device__ __forceinline__ void rr_children(const DevParams &P, unsigned c0, unsigned c1, int L, R &f) {
    using io = row_io<LPI, R>;
    for (unsigned c = c0; c < c1; c += RR_NB) {
        R r[RR_NB];
        float v[RR_NB];
#pragma unroll
        for (int q = 0; q < RR_NB; q++) {
            const bool in = c + q < c1;
            r[q] = in ? io::load(P.W, P.user_off + P.feat_user.index[c + q], P.pitch, L, P.k) : row_traits<R>::zero();
            v[q] = in ? P.feat_user.value[c + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < RR_NB; q++)
            if (c + q < c1) axpy4(f, r[q], v[q]);
    }
}

// LINES = false: the row of section 6y, feedback sum + W_user[sec_user] * 1.  LINES = true (section 6z): the section brings a USER line
// of (id, value) entries instead of one user -- behind the feedback sum (0 without lists), per entry in line order W_user[uid] * val,
// then the children of uid in the feature_user table, unscaled by val and not followed further (k_rank_user, apex_svd_base.h:731-734).
// The child ranges of a batch's entries are fetched with its rows: a child's row load depends on the table words.
template <int LPI, typename R, bool LINES>
__global__ __launch_bounds__(256) void k_rank_live_rows(const DevParams P, const RankLiveRowsDev D) {
    using io = row_io<LPI, R>;
    constexpr int SPW = 64 / LPI;   // sections of a wave
    const int lane = threadIdx.x & 63, L = lane & (LPI - 1);
    const long sec = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * SPW + lane / LPI;
    if (sec >= D.nsec) return;
    const bool lists = !LINES || D.fb_p0 != nullptr;
    const int b = lists ? D.fb_p0[sec] : 0, e = lists ? D.fb_p0[sec + 1] : 0;
    R urow;
    if (!LINES) urow = io::load(P.W, P.user_off + D.sec_user[sec], P.pitch, L, P.k);   // in flight under the whole list
    R f = row_traits<R>::zero();
    for (int t = b; t < e; t += RR_NB) {
        R r[RR_NB];
        float v[RR_NB];
#pragma unroll
        for (int q = 0; q < RR_NB; q++) {
            const bool in = t + q < e;
            r[q] = in ? io::load(P.W, P.fb_off + D.fb_index[t + q], P.pitch, L, P.k) : row_traits<R>::zero();
            v[q] = in ? D.fb_value[t + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < RR_NB; q++)
            if (t + q < e) {   // a row past the list is not added: x + 0 * 0 is not x for x = -0
                axpy4(f, r[q], v[q]);
                if (v[q] != v[q]) rr_poison(f, v[q]);
            }
    }
    if (!LINES) {
        axpy4(f, urow, 1.0f);   // proc_user on top of tmp_ufeedback: the USER line u:1
    } else {
        const int le = D.ul_p0[sec + 1];
        for (int t = D.ul_p0[sec]; t < le; t += RR_NB) {
            R r[RR_NB];
            float v[RR_NB];
            unsigned c0[RR_NB], c1[RR_NB];
#pragma unroll
            for (int q = 0; q < RR_NB; q++) {
                const bool in = t + q < le;
                const unsigned uid = in ? D.ul_index[t + q] : 0u;
                const bool kids = in && uid < P.feat_user.num_row;   // ids at or past the table's rows have no children
                r[q] = in ? io::load(P.W, P.user_off + uid, P.pitch, L, P.k) : row_traits<R>::zero();
                v[q] = in ? D.ul_value[t + q] : 0.0f;
                c0[q] = kids ? P.feat_user.row_ptr[uid] : 0u;
                c1[q] = kids ? P.feat_user.row_ptr[uid + 1] : 0u;
            }
#pragma unroll
            for (int q = 0; q < RR_NB; q++)
                if (t + q < le) {
                    axpy4(f, r[q], v[q]);
                    if (v[q] != v[q]) rr_poison(f, v[q]);   // a NaN VALUE of the line: as a NaN feedback value above
                    rr_children<LPI, R>(P, c0[q], c1[q], L, f);
                }
        }
    }
    io::store(D.rows, (size_t)sec, P.pitch, L, P.k, f);
}

void launch_rank_live_rows(const DevParams &P, const RankLiveRowsDev &D, hipStream_t st) {
    if (D.nsec <= 0) return;
    SVDF_DISPATCH_ROW(P.k, {
        const long per_block = 4L * (64 / LPI);
        const dim3 grid((unsigned)((D.nsec + per_block - 1) / per_block));
        if (D.ul_p0) hipLaunchKernelGGL((k_rank_live_rows<LPI, R, true>), grid, dim3(256), 0, st, P, D);
        else hipLaunchKernelGGL((k_rank_live_rows<LPI, R, false>), grid, dim3(256), 0, st, P, D);
    });
}

// The prepared item matrix and bias vector of a trainer with a feature_item table (section 6z), once per call: for every item i
//   f = 0; f += W_item[i] * 1; per child c of i in table order: f += W_item[cid] * (float)((double)cval * 1.0)
//   b = 0 + i_bias[i] * 1;     per child:                        b = b + i_bias[cid] * cval * 1
// -- rank_prepare_item (svdf_k_rank.hip) for an ITEM line i:1 without global features, operation for operation.  One lane group per item,
// grid-stride; the lane groups of a wave differ only in their trip counts.  item_rows has W_item's layout ([num_item][pitch], pads 0).
template <int LPI, typename R>
__global__ __launch_bounds__(256) void k_rank_live_items(const DevParams P, float *item_rows, float *item_bias) {
    using io = row_io<LPI, R>;
    constexpr int IPW = 64 / LPI;
    const int lane = threadIdx.x & 63, L = lane & (LPI - 1);
    const long first = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * IPW + lane / LPI;
    const long stride = (long)gridDim.x * (blockDim.x >> 6) * IPW;
    for (long i = first; i < (long)P.num_item; i += stride) {
        const bool kids = (unsigned long)i < (unsigned long)P.feat_item.num_row;
        const unsigned c0 = kids ? P.feat_item.row_ptr[i] : 0u, c1 = kids ? P.feat_item.row_ptr[i + 1] : 0u;
        R f = row_traits<R>::zero();
        axpy4(f, io::load(P.W, P.item_off + (size_t)i, P.pitch, L, P.k), 1.0f);
        float bias = 0.0f + P.bias[P.item_off + i] * 1.0f;
        for (unsigned c = c0; c < c1; c += RR_NB) {
            R r[RR_NB];
            float v[RR_NB], cb[RR_NB];
#pragma unroll
            for (int q = 0; q < RR_NB; q++) {
                const bool in = c + q < c1;
                const unsigned cid = in ? P.feat_item.index[c + q] : 0u;
                r[q] = in ? io::load(P.W, P.item_off + cid, P.pitch, L, P.k) : row_traits<R>::zero();
                v[q] = in ? P.feat_item.value[c + q] : 0.0f;
                cb[q] = in ? P.bias[P.item_off + cid] : 0.0f;
            }
#pragma unroll
            for (int q = 0; q < RR_NB; q++)
                if (c + q < c1) {
                    axpy4(f, r[q], (float)((double)v[q] * 1.0));
                    bias = bias + cb[q] * v[q] * 1.0f;
                }
        }
        io::store(item_rows, (size_t)i, P.pitch, L, P.k, f);
        if (L == 0) item_bias[i] = bias;
    }
}

void launch_rank_live_items(const DevParams &P, float *item_rows, float *item_bias, hipStream_t st) {
    if (P.num_item <= 0) return;
    SVDF_DISPATCH_ROW(P.k, {
        const long per_block = 4L * (64 / LPI);
        const long blocks = std::min<long>(((long)P.num_item + per_block - 1) / per_block, 8192);
        hipLaunchKernelGGL((k_rank_live_items<LPI, R>), dim3((unsigned)blocks), dim3(256), 0, st, P, item_rows, item_bias);
    });
}

}  // namespace svdf

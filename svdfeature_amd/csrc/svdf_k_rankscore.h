// svdf_k_rankscore.h -- the score of one candidate for one user on the live model, shared by the batch ranking kernels
// (svdf_k_rankeval.hip, svdf_k_ranktopn.hip; DESIGN.md sections 6w, 6x): i_bias[i] + <W_user[u], W_item[i]> in the ranker's fp32 order.
#ifndef SVDF_K_RANKSCORE_H_
#define SVDF_K_RANKSCORE_H_

#include "svdf_kernels.h"

namespace svdf {

// The order in two parts, for a kernel that walks K in chunks (svdf_k_ranktopn_exact.hip): the four serial chains over n consecutive full
// float4s of both rows, carried in `a` from chunk to chunk ...
__device__ __forceinline__ void re_row_chains(float4 &a, const float4 *__restrict__ p4, const float4 *__restrict__ q4, int n) {
    for (int j = 0; j < n; j++) {
        const float4 p = p4[j], v = q4[j];
        a.x = a.x + p.x * v.x; a.y = a.y + p.y * v.y; a.z = a.z + p.z * v.z; a.w = a.w + p.w * v.w;
    }
}
// ... and the end: (a0 + a2) + (a1 + a3), the ntail (0 .. 3) elements of the rows' last float4s p, v in index order, the bias
__device__ __forceinline__ float re_row_finish(const float4 &a, int ntail, const float4 &p, const float4 &v, float bias) {
    float sum = (a.x + a.z) + (a.y + a.w);
    if (ntail) {
        sum = sum + p.x * v.x;
        if (ntail > 1) sum = sum + p.y * v.y;
        if (ntail > 2) sum = sum + p.z * v.z;
    }
    return 0.0f + (bias + sum);   // k_rank_score: item_score (0) + (bias + dot)
}
// one candidate against one user by ONE lane, both rows row-major in HBM
__device__ __forceinline__ float re_row_score(int k, const float4 *__restrict__ p4, const float4 *__restrict__ q4, float bias) {
    const int nfull = k >> 2, ntail = k & 3;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p = a, v = a;
    re_row_chains(a, p4, q4, nfull);
    if (ntail) { p = p4[nfull]; v = q4[nfull]; }
    return re_row_finish(a, ntail, p, v, bias);
}
__device__ __forceinline__ const float4 *re_user_row(const DevParams &P, unsigned u) {
    return reinterpret_cast<const float4 *>(P.W + (size_t)(P.user_off + u) * P.pitch);
}
// the user row section `sec` of a piece scores with: row `sec` of the workspace k_rank_live_rows wrote (a user-group trainer: feedback sum + user
// row), or the W_user row of the section's user
__device__ __forceinline__ const float4 *re_section_row(const DevParams &P, const float *user_rows, const unsigned *sec_user, int sec) {
    return user_rows ? reinterpret_cast<const float4 *>(user_rows + (size_t)sec * P.pitch) : re_user_row(P, sec_user[sec]);
}
// the item side a call scores with: W_item / i_bias where the model keeps them, or the matrix and bias vector k_rank_live_items prepared
// (a trainer with a feature_item table) -- both [num_item][pitch] / [num_item].  ONE select per kernel, outside
// its scoring loops
__device__ __forceinline__ const float *re_item_base(const DevParams &P, const float *item_rows) {
    return item_rows ? item_rows : P.W + (size_t)P.item_off * P.pitch;
}
__device__ __forceinline__ const float *re_item_bias(const DevParams &P, const float *item_bias) { return item_bias ? item_bias : P.bias + P.item_off; }
__device__ __forceinline__ const float4 *re_item_row(const float *item_base, int pitch, long i) {
    return reinterpret_cast<const float4 *>(item_base + (size_t)i * pitch);
}

}  // namespace svdf
#endif

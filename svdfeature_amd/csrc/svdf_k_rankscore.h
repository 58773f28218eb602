// svdf_k_rankscore.h -- the score of one candidate for one user on the live model, shared by the batch ranking kernels
// (svdf_k_rankeval.hip, svdf_k_ranktopn.hip; DESIGN.md sections 6w, 6x): i_bias[i] + <W_user[u], W_item[i]> in the ranker's fp32 order.
#ifndef SVDF_K_RANKSCORE_H_
#define SVDF_K_RANKSCORE_H_

#include "svdf_kernels.h"

namespace svdf {

// one candidate against one user by ONE lane, both rows row-major in HBM
__device__ __forceinline__ float re_row_score(int k, const float4 *__restrict__ p4, const float4 *__restrict__ q4, float bias) {
    const int nfull = k >> 2, ntail = k & 3;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (int j = 0; j < nfull; j++) {
        const float4 p = p4[j], v = q4[j];
        a0 = a0 + p.x * v.x; a1 = a1 + p.y * v.y; a2 = a2 + p.z * v.z; a3 = a3 + p.w * v.w;
    }
    float sum = (a0 + a2) + (a1 + a3);
    if (ntail) {
        const float4 p = p4[nfull], v = q4[nfull];
        sum = sum + p.x * v.x;
        if (ntail > 1) sum = sum + p.y * v.y;
        if (ntail > 2) sum = sum + p.z * v.z;
    }
    return 0.0f + (bias + sum);   // k_rank_score: item_score (0) + (bias + dot)
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

// svdf_foldin.cpp -- fold-in on the live model: the host side of svdf_fold_in -- the refusals, the arguments
// through svdf_foldin_lists.h, one packed upload, one launch of k_fold_in (svdf_k_foldin.hip), the rows back.
#include <svdfeature_amd.h>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_foldin_lists.h"

namespace svdf {

void Engine::fold_in(long S, const unsigned *user, const int64_t *ptr, const unsigned *item, const float *label, float reg, int write, float *rows_out) {
    // ---- the configuration: the rule is the linear link's prediction without its factor term, on a model whose score has no other part
    if (mtype_.active_type != ACT_LINEAR) fail("fold_in: active_type != 0 is not covered: the rule solves the linear link's least squares");
    rank_live_refusals("fold_in", true);   // extend_type 2 / 15, side tables, common_latent_space, amd:gpus > 1, rank handles, no model
    if (user_group()) fail("fold_in: user-group trainers (format_type = 1) are not covered: the score has a feedback part");
    if (mp_.num_factor > FOLD_IN_MAX_FACTOR) fail("fold_in: num_factor must be at most 128");
    // ---- the arguments, before any device work
    const int64_t n = fold_in_validate(S, user, ptr, item, label, reg, write, rows_out, (long)mp_.num_user, (long)mp_.num_item);
    if (S == 0) return;   // nothing to solve: no device is asked for
    need_device("fold_in");
    flush();   // behind whatever has been staged
    const DevParams &P = params();
    FoldInPack in;
    fold_in_pack(S, user, ptr, item, label, n, in);
    reserve_or_fail("fold_in", fi_in_, in.words.size(), "the sections' ratings");
    fi_in_.upload(in.words.data(), in.words.size(), stream_);
    const size_t nout = (size_t)S * (size_t)P.k;
    reserve_or_fail("fold_in", fi_out_, nout, "the rows");
    FoldInDev D;
    D.nsec = S;
    D.ptr = fi_in_.p;
    const unsigned *w4 = reinterpret_cast<const unsigned *>(fi_in_.p);
    D.user = w4 + in.o_user;
    D.item = w4 + in.o_item;
    D.label = reinterpret_cast<const float *>(w4 + in.o_label);
    D.reg = reg;
    D.write = write ? 1 : 0;
    D.rows_out = fi_out_.p;
    launch_fold_in(P, D, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
    HIPCHECK(hipMemcpyAsync(rows_out, fi_out_.p, nout * sizeof(float), hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));
    n_fold_in_sections_ += S;
}

}  // namespace svdf

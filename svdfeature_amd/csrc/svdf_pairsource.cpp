// svdf_pairsource.cpp -- passes of rank pairs from positives only: the host side of svdf_pair_source_create /
// svdf_dataset_from_pair_source / svdf_pair_source_draw.  A source keeps its rows and every user's distinct items in HBM (one upload each
// at creation, svdf_pairsource_lists.h builds the lists); a pass draws its negatives there (svdf_k_pairdraw.hip) into three columns of
// n * num_neg entries and is built from those columns where Engine::dataset_from_pairs has a route that starts from device columns -- the
// window sequence of svdf_wseq.cpp (section 6v's builder) and the exact level schedule of schedule_device_columns.  Everything else copies
// the columns back and IS dataset_from_pairs on them, so no result depends on the route.  A HARD pass (section 6ad, svdf_k_pairhard.hip:
// the best of num_cand candidates by live score) differs in the step that fills the columns and in what it admits, and in nothing else.
// A WEIGHTED source (section 6ae) also keeps the running sums of its item weights and their guide table (svdf_pairweight_lists.h); both
// kernels then draw through those tables, and nothing else about a pass changes.  A SHUFFLED pass (section 6af) takes an order_seed: one more
// kernel (svdf_k_pairorder.hip) gathers the rows in the order sigma (svdf_pairorder_lists.h) before the draw, and the route is decided on
// the permuted order.
#include <svdfeature_amd.h>

#include <memory>

#include "svdf_internal.h"
#include "svdf_kernels.h"
#include "svdf_pairhard_lists.h"

namespace svdf {

template <typename T>
static void pair_src_reserve(DevBuf<T> &buf, size_t n, const char *what) {   // (in either error mode: fail() prints or throws what it is given)
    const hipError_t e = buf.try_reserve(n);
    if (e != hipSuccess)
        fail(std::string("pair_source: ") + what + " of " + std::to_string(n * sizeof(T)) + " bytes could not be allocated: " + hipGetErrorString(e) + " at hipMalloc");
}

PairSource::~PairSource() {
    if (owner) owner->pair_source_forget(this);
}
void Engine::pair_source_forget(PairSource *src) {
    pair_sources_.erase(std::remove(pair_sources_.begin(), pair_sources_.end(), src), pair_sources_.end());   // (every draw has been waited for)
}

PairSource *Engine::pair_source_create(long n, const unsigned *user, const unsigned *pos, const unsigned *item_weight) {
    check(trainer_ready_, "pair_source: call init_model / load_model and init_trainer first");
    // ---- the rows, the weights and the lists, before any device work
    PairSrcLists L;
    PairWeightLists Wt;
    if (item_weight) pair_weight_source((long)mp_.num_user, (long)mp_.num_item, n, user, pos, item_weight, L, Wt);
    else {
        pair_src_check_rows((long)mp_.num_user, (long)mp_.num_item, n, user, pos);
        pair_src_build((long)mp_.num_user, (long)mp_.num_item, n, user, pos, L, pair_src_threads(n));
    }
    std::unique_ptr<PairSource> src(new PairSource());
    src->n = n;
    src->weighted = item_weight != nullptr;
    if (src->weighted) { src->weight_sum = Wt.cdf.back(); src->weight_shift = Wt.shift; }
    for (long r = 1; r < n; r++) src->same += user[r] == user[r - 1];
    if (!host_only_) {   // (a host-only handle's source reaches every refusal of a pass, then "needs a GPU")
        need_device("pair_source");
        pair_src_reserve(src->user, (size_t)n, "the user column");
        pair_src_reserve(src->pos, (size_t)n, "the item column");
        pair_src_reserve(src->uptr, L.uptr.size(), "the list offsets");
        pair_src_reserve(src->uitems, std::max<size_t>(L.uitems.size(), 1), "the users' item lists");
        src->user.upload(user, (size_t)n, stream_);
        src->pos.upload(pos, (size_t)n, stream_);
        src->uptr.upload(L.uptr.data(), L.uptr.size(), stream_);
        src->uitems.upload(L.uitems.data(), L.uitems.size(), stream_);
        if (src->weighted) {
            pair_src_reserve(src->cdf, Wt.cdf.size(), "the item weights' running sums");
            pair_src_reserve(src->guide, Wt.guide.size(), "the item weights' guide table");
            src->cdf.upload(Wt.cdf.data(), Wt.cdf.size(), stream_);
            src->guide.upload(Wt.guide.data(), Wt.guide.size(), stream_);
        }
        HIPCHECK(hipStreamSynchronize(stream_));   // L and Wt go out of scope
    }
    src->owner = this;
    pair_sources_.push_back(src.get());
    return src.release();
}

// The step that fills a pass's columns, and the only one that differs between the plain pass (num_cand = 0: k_pair_draw) and the hard one
// (section 6ad: k_pair_hard draws num_cand candidates per pair, scores them with the model as every call issued earlier on the trainer's
// stream leaves it, and keeps the best).  With an ORDER (section 6af) k_pair_order runs first: it gathers the source's rows in the order
// sigma into two scratch columns, which the draw kernels then read in place of the source's -- they are launched as they are without one --,
// and counts the adjacent positions that share their user into *same_out.  Its flag and count come back with the draw's flag.
void Engine::pair_source_launch(const PairSource &src, int num_neg, int num_cand, uint64_t seed, unsigned *d_user, unsigned *d_pos, unsigned *d_neg,
                                float *d_score, const uint64_t *order, long *same_out) {
    DevBuf<unsigned> flag, ou, op;   // flag[0] the draw's; with an order flag[1] the walk's and flag[2] the count
    const size_t words = order ? 3 : 1;
    pair_src_reserve(flag, words, "the flag");
    HIPCHECK(hipMemsetAsync(flag.p, 0, words * sizeof(unsigned), stream_));
    if (order) {
        pair_src_reserve(ou, (size_t)src.n, "the user column of a shuffled pass");
        pair_src_reserve(op, (size_t)src.n, "the item column of a shuffled pass");
        PairOrderDev O;
        O.n = src.n;
        O.K = pair_order_keys(*order, src.n);
        O.user = src.user.p; O.pos = src.pos.p;
        O.out_user = ou.p; O.out_pos = op.p;
        O.flag = flag.p + 1; O.same = flag.p + 2;
        launch_pair_order(O, stream_);
        HIPCHECK(hipGetLastError());
        n_launches_++;
    }
    PairHardDev H;
    PairDrawDev &D = H.D;
    D.npair = src.n * (long)num_neg;
    D.num_neg = num_neg;
    D.seed = seed;
    D.num_item = (unsigned)mp_.num_item;
    D.user = order ? ou.p : src.user.p; D.pos = order ? op.p : src.pos.p; D.uptr = src.uptr.p; D.uitems = src.uitems.p;
    D.out_user = d_user; D.out_pos = d_pos; D.out_neg = d_neg;
    D.flag = flag.p;
    H.num_cand = num_cand; H.out_score = d_score;
    PairWeightDev T;   // (without weights: no table, the uniform kernels)
    if (src.weighted) { T.cdf = src.cdf.p; T.guide = src.guide.p; T.W = src.weight_sum; T.num_item = D.num_item; T.shift = src.weight_shift; }
    if (num_cand > 0) {
        flush();   // behind whatever has been staged
        launch_pair_hard(params(), H, T, (int)pair_weight_form_, (int)pair_hard_form_, stream_);
    } else launch_pair_draw(D, T, (int)pair_weight_form_, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
    unsigned spent[3] = {0, 0, 0};
    HIPCHECK(hipMemcpyAsync(spent, flag.p, words * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));   // (the scratch columns have been read)
    if (spent[1]) fail(pair_order_spent(*order, (long)spent[1] - 1));
    if (spent[0]) fail("pair_source: pair " + std::to_string((long)spent[0] - 1) + " found no negative in " + std::to_string(PAIR_SRC_DRAWS) + " draws");
    if (same_out) *same_out = order ? (long)spent[2] : src.same;
}

// what every pass refuses, on the host, before any device work.  A hard pass scores with svdf_rank_topn's kernels' arithmetic on the
// trainer's own rows: its trainer is one that call admits (rank_live_refusals: format_type = 0, extend_type = 0, no side tables, one GPU).
void Engine::pair_source_admit(const PairSource *src, int num_neg, int num_cand) {
    if (!src) fail("pair_source: bad arguments");
    if (src->owner != this) fail("pair_source: the source was created on another trainer");
    if (num_cand == 0) { pair_src_check_pass(src->n, num_neg); return; }
    pair_hard_check_pass(src->n, num_neg, num_cand);
    rank_live_refusals("pair_source");
}

void Engine::pair_source_draw(PairSource *src, int num_neg, uint64_t seed, unsigned *neg_out, int num_cand, float *score_out, const uint64_t *order,
                              unsigned *user_out, unsigned *pos_out) {
    pair_source_admit(src, num_neg, num_cand);
    check(neg_out != nullptr && (!order || (user_out && pos_out)), "pair_source: bad arguments");
    need_device("pair_source");
    const size_t N = (size_t)src->n * (size_t)num_neg;
    DevBuf<unsigned> neg, cu, cp;
    DevBuf<float> score;
    pair_src_reserve(neg, N, "the negative column of a pass");
    if (score_out) pair_src_reserve(score, N, "the score column of a pass");
    if (order) {   // a caller of the shuffled draw needs the pass's own user and item columns to know which row a negative belongs to
        pair_src_reserve(cu, N, "the user column of a pass");
        pair_src_reserve(cp, N, "the positive column of a pass");
    }
    pair_source_launch(*src, num_neg, num_cand, seed, cu.p, cp.p, neg.p, score_out ? score.p : nullptr, order);
    HIPCHECK(hipMemcpyAsync(neg_out, neg.p, N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    if (score_out) HIPCHECK(hipMemcpyAsync(score_out, score.p, N * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (order) {
        HIPCHECK(hipMemcpyAsync(user_out, cu.p, N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(pos_out, cp.p, N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    }
    HIPCHECK(hipStreamSynchronize(stream_));
}

Dataset *Engine::dataset_from_pair_source(PairSource *src, int num_neg, uint64_t seed, int num_cand, const uint64_t *order) {
    pair_source_admit(src, num_neg, num_cand);
    check(trainer_ready_, "dataset: init_trainer has not been called");
    need_device("dataset");
    const long N = src->n * (long)num_neg;
    // ---- the route, in the order of dataset_from_pairs' own decisions on the same columns
    const bool one_gpu = !multi_ && !is_peer_ && !in_multi_scope();
    const bool to_windows = single_minibatch() && !user_group() && window_rows_allowed();          // where it takes wseq_from_pairs
    const bool windows_hbm = one_gpu && to_windows && device_window_ready() && wseq_pair_sub_ == 0;
    // the pretest of punit_dataset_from_pairs on the EXPANDED user column: the num_neg pairs of a row are adjacent
    // -- with an order on the PERMUTED rows: the adjacent positions that share their user are counted by k_pair_order, so these two wait for it
    const bool units_ok = punit_config_ok() && N >= 2 && N < 0x7FFFFFF0L;
    const bool exact_ok = one_gpu && !to_windows && !auto_step_active() && device_sched_ && fused_allowed() && !user_group() && !relaxed();
    // ---- what dataset_from_pairs refuses about the trainer whatever the columns hold, in its own words, before any device work
    if (wseq_pair_sub_ > 0 && ((multi_ && !in_multi_scope()) || (single_minibatch() && (user_group() || window_rows_allowed())))) wseq_pair_check("dataset_from_pairs");
    if (!(multi_ && !in_multi_scope())) resident_rows_check();   // (a user-group trainer's pairs end in dataset_from_csr)
    DevBuf<unsigned> cu, cp, cq;
    pair_src_reserve(cu, (size_t)N, "the user column of a pass");
    pair_src_reserve(cp, (size_t)N, "the positive column of a pass");
    pair_src_reserve(cq, (size_t)N, "the negative column of a pass");
    long same = 0;
    pair_source_launch(*src, num_neg, num_cand, seed, cu.p, cp.p, cq.p, nullptr, order, &same);
    const bool to_units = units_ok && 2 * (src->n * (long)(num_neg - 1) + same) >= N;
    const bool exact_hbm = exact_ok && !to_units;
    if (!windows_hbm && !exact_hbm) {   // dataset_from_pairs itself, on the columns copied back
        std::vector<unsigned> hu((size_t)N), hp((size_t)N), hq((size_t)N);
        HIPCHECK(hipMemcpyAsync(hu.data(), cu.p, (size_t)N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(hp.data(), cp.p, (size_t)N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipMemcpyAsync(hq.data(), cq.p, (size_t)N * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        cu.release(); cp.release(); cq.release();
        Dataset *ds = dataset_from_pairs(N, hu.data(), hp.data(), hq.data());
        n_pair_src_fallback_++;
        n_pair_src_hard_ += num_cand > 0;
        n_pair_src_weighted_ += src->weighted;
        n_pair_src_shuffled_ += order != nullptr;
        return ds;
    }
    if (windows_hbm) {   // section 6v's builder on the pos / neg columns as drawn: item counts, window rule and windows from where they are
        Dataset *seq = wseq_from_device_pairs(N, cu.p, cp.p, nullptr, cq.p);
        if (!seq) fail("pair_source: the drawn columns hold an id the windows refuse");   // (validated ids, pos != neg: not reached)
        n_pair_src_hbm_++;
        n_pair_src_hard_ += num_cand > 0;
        n_pair_src_weighted_ += src->weighted;
        n_pair_src_shuffled_ += order != nullptr;
        return seq;
    }
    // ---- the merged, index-sorted form the level schedule starts from: lower / higher item id and the entries' signs (pos != neg by the rule)
    DevBuf<unsigned> lo_, hi_, flag;
    DevBuf<float> vlo, vhi, one;
    pair_src_reserve(lo_, (size_t)N, "a schedule column"); pair_src_reserve(hi_, (size_t)N, "a schedule column");
    pair_src_reserve(vlo, (size_t)N, "a schedule column"); pair_src_reserve(vhi, (size_t)N, "a schedule column");
    pair_src_reserve(one, (size_t)N, "a schedule column"); pair_src_reserve(flag, 1, "the flag");
    HIPCHECK(hipMemsetAsync(flag.p, 0, sizeof(unsigned), stream_));
    launch_pairs_prepare(N, cp.p, cq.p, lo_.p, hi_.p, vlo.p, vhi.p, one.p, flag.p, stream_);
    HIPCHECK(hipGetLastError());
    cp.release(); cq.release();   // (stream-ordered frees: the kernel above has been enqueued)
    std::unique_ptr<Dataset> ds(new Dataset());
    adopt(ds.get()); ds->num_row = N; ds->kind = 2;
    const unsigned *res[3] = {cu.p, lo_.p, hi_.p};
    const unsigned off[3] = {0u, (unsigned)mp_.num_user, (unsigned)mp_.num_user};
    const unsigned limit[3] = {(unsigned)mp_.num_user, (unsigned)mp_.num_item, (unsigned)mp_.num_item};
    const char *msg[3] = {"user feature index exceed bound", "item feature index exceed bound", "item feature index exceed bound"};
    const unsigned *key = sort_batches_ == 1 ? lo_.p : (sort_batches_ == 2 ? cu.p : nullptr);
    FusedDev &f = ds->fused;
    f.max_nu = 1; f.max_ni = 2; f.has_g = false; f.inline_g = false;
    schedule_device_columns(ds.get(), N, 3, res, off, limit, msg, key, sort_batches_ == 1 ? limit[1] : limit[0],
                            {DUCol{cu.p, &f.uidx[0]}, DUCol{lo_.p, &f.iidx[0]}, DUCol{hi_.p, &f.iidx[1]}},
                            {DFCol{one.p, &f.label}, DFCol{one.p, &f.uval[0]}, DFCol{vlo.p, &f.ival[0]}, DFCol{vhi.p, &f.ival[1]}});
    const long nb2 = (mp_.no_user_bias ? 0 : 1) + 2;
    ds->algorithmic_bytes = N * (8L * mp_.num_factor * 3 + 8 * nb2 + 16 + 8 * 3);
    n_pair_src_hbm_++;
    n_pair_src_hard_ += num_cand > 0;
    n_pair_src_weighted_ += src->weighted;
    n_pair_src_shuffled_ += order != nullptr;
    return ds.release();
}

// The probe svdf_pair_weight_lookup on a trainer: the tables of (num_item, item_weight) built and validated as a weighted source builds them,
// uploaded, and the map of k_pair_draw / k_pair_hard run on the caller's words in one small launch.
void Engine::pair_weight_lookup(long num_item, const unsigned *item_weight, int form, long nx, const uint64_t *x, unsigned *id_out) {
    check(form >= 0 && form <= 2 && nx >= 0 && (nx == 0 || (x && id_out)), "pair_weight_lookup: bad arguments");
    PairWeightLists Wt;
    pair_weight_build(num_item, item_weight, Wt);
    need_device("pair_weight_lookup");
    if (nx == 0) return;
    DevBuf<unsigned> cdf, guide, ids;
    DevBuf<uint64_t> words;
    pair_src_reserve(cdf, Wt.cdf.size(), "the item weights' running sums");
    pair_src_reserve(guide, Wt.guide.size(), "the item weights' guide table");
    pair_src_reserve(words, (size_t)nx, "the words");
    pair_src_reserve(ids, (size_t)nx, "the ids");
    cdf.upload(Wt.cdf.data(), Wt.cdf.size(), stream_);
    guide.upload(Wt.guide.data(), Wt.guide.size(), stream_);
    words.upload(x, (size_t)nx, stream_);
    PairWeightDev T = Wt.view();
    T.cdf = cdf.p; T.guide = guide.p;
    launch_pair_weight_lookup(T, form == 0 ? (int)pair_weight_form_ : form, nx, words.p, ids.p, stream_);
    HIPCHECK(hipGetLastError());
    n_launches_++;
    HIPCHECK(hipMemcpyAsync(id_out, ids.p, (size_t)nx * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    HIPCHECK(hipStreamSynchronize(stream_));
}

}  // namespace svdf

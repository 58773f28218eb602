"""The HIP engine against the oracle on models at the edges of float32 (run with -m gpu on an MI355X): denormal rows, exact zeros of both signs,
rows that overflow to inf and NaN, saturated sigmoid links -- the strata of tests/float_edges.py, whose inputs tests/test_float_edges.py proves on
the CPU -- through the staged kernels at every lane-group shape, the resident data sets under each kernel routing, lazy decay, the window step
against its checker steps, and the scoring calls.

Bar: fe.same_bits_or_nan on W_user, W_item, u_bias, i_bias, g_bias (W_ufeedback and ufeedback_bias where the trainer has them) and on the
predictions: every bit of every value that is not a NaN, and NaN at the same positions.  Each case asserts the data set kind or the counter that
shows its route ran.  One pass per case, a few thousand rows."""
import numpy as np
import pytest

import float_edges as fe
import svdfeature_amd as sa
from oracle import oracle

pytestmark = pytest.mark.gpu


def _hip(f, a, e):
    return sa.Trainer(f, a, e)


def _rows(b):
    return sum(x.data.num_row for x in b[1]) if b[0] == "blocks" else b[1].num_row if b[0] == "rows" else len(b[1])


def _dataset(t, b):
    if b[0] == "triples":
        return t.dataset_from_triples(b[1], b[2], b[3])
    if b[0] == "pairs":
        return t.dataset_from_pairs(b[1], b[2], b[3])
    if b[0] == "rows":
        return t.dataset_from_csr(b[1])
    return t.dataset_from_blocks(b[1])


def _check_counters(t, c, counters):
    for what, want in counters:
        got = t.counter(what)
        if want == "rows":
            want = sum(_rows(b) for b in c.batches)
        assert (got > 0) if want == ">0" else (got == want), "counter %d is %d, expected %s" % (what, got, want)


def _check_model(t, c, want, what):
    for name in c.model:
        fe.same_bits_or_nan(t.view(name), want[name], "%s: %s" % (what, name))


def _check_dataset_scores(t, c, b, ds, want_pred, what):
    """predict_dataset: file order, every row; eval_dataset: the evaluator's sum over the same predictions"""
    got = t.predict_dataset(ds)
    if b[0] == "blocks" and c.extend == 0:   # (predict_block answers for DEFAULT blocks)
        got = got[np.concatenate([np.full(x.data.num_row, x.extend_tag == 0) for x in b[1]])]
    fe.same_bits_or_nan(got, want_pred, what + ": predict_dataset")
    if b[0] != "blocks":
        label = c.csr(b).row_label
        s, n = t.eval_dataset(ds)
        ref = oracle.sum_sq_err(want_pred, label)
        assert n == len(label)
        if np.isfinite(ref):   # the sum is a double over at most 5 000 terms: any order agrees to n * 2^-53
            assert abs(s - ref) <= 1e-12 * abs(ref), (s, ref)
        else:
            assert np.isnan(s) == np.isnan(ref) and (np.isnan(ref) or s == ref), (s, ref)


@pytest.mark.parametrize("route", fe.ROUTES, ids=lambda r: r.id)
def test_the_engine_equals_the_oracle_at_the_float_edges(route):
    c, want = route.case, route.expected()
    conf = list(route.conf)
    if route.mode == "window":
        conf += [("amd:step", "minibatch"), ("amd:window", str(-(-_rows(c.batches[0]) // route.kw["windows"])))]
    t = fe.fresh(c, _hip, conf=conf, knobs=route.knobs)
    dss = []
    if route.mode == "staged":
        fe.train(t, c)
    else:
        dss = [_dataset(t, b) for b in c.batches]
        if route.kinds is not None:
            assert [ds.kind for ds in dss] == route.kinds, [ds.kind for ds in dss]
        if route.mode == "window":
            assert dss[0].num_batches == route.kw["windows"]
            if route.kw.get("sub"):   # the ordered sub-steps have work: in every window some item has more rows than one sub-step takes
                item, n = c.batches[0][2], _rows(c.batches[0])
                for w in range(route.kw["windows"]):
                    assert np.bincount(item[n * w // route.kw["windows"]:n * (w + 1) // route.kw["windows"]]).max() > route.kw["sub"]
        if "use_simple_units" in dict(route.knobs):   # SVD++ units on the register-resident fast path, or none of them
            assert (dss[0].num_simple_units > 0) == bool(dict(route.knobs)["use_simple_units"])
        for ds in dss:
            t.train_dataset(ds)
        t.synchronize()
    _check_counters(t, c, route.counters)
    _check_model(t, c, want, route.id)
    fe.same_bits_or_nan(fe.scores(t, c), want["pred"], route.id + ": predict_batch / predict_block")
    at = 0
    for b, ds in zip(c.batches, dss):
        n = sum(x.data.num_row for x in b[1] if x.extend_tag == 0 or c.extend == 2) if b[0] == "blocks" else _rows(b)
        _check_dataset_scores(t, c, b, ds, want["pred"][at:at + n], route.id)
        at += n
    for ds in dss:
        ds.close()
    t.close()


@pytest.mark.parametrize("trained", [0, 1], ids=["as_set", "after_a_pass"])
@pytest.mark.parametrize("stratum,variant", [("denormal", None), ("zeros", 3)])
def test_ranking_on_denormal_and_zero_models(stratum, variant, trained):
    """svdf_rank_topn and svdf_rank_eval_positions against the numpy float32 rule of tests/test_rank_topn.py (IEEE denormals in numpy): on the
    arrays as set the scores are denormal (denormal: bias + a dot product that underflows) or tie at +-0 by the dozen (zeros: all-zero rows
    and biases of both signs), and the ties must still break by id; after a pass the same on what the kernels left"""
    from test_rank_topn import rule_topn
    c = fe.case("triples", stratum, 64, variant)
    t = fe.fresh(c, _hip, knobs=fe.PLAIN)
    if trained:
        ds = _dataset(t, c.batches[0])
        t.train_dataset(ds)
        t.synchronize()
    U, W, bias = t.view("W_user").copy(), t.view("W_item").copy(), t.view("i_bias").copy()
    rng = np.random.default_rng(5)
    S, ni, top_n = 40, W.shape[0], 200
    users = rng.integers(0, U.shape[0], S).astype(np.uint32)
    users[:4] = [0, 1, 7, 8]   # (zeros: an all +0 row, an all -0 row)
    ban = [rng.permutation(ni)[:int(rng.integers(0, 21))].astype(np.uint32) for _ in range(S)]
    ban_ptr, ban_item = np.concatenate([[0], np.cumsum([len(b) for b in ban])]).astype(np.int64), np.concatenate(ban)
    want = rule_topn(U, W, bias, users, top_n, ban_ptr, ban_item)
    before = t.counter(39)
    items, scores, count, nan = t.rank_topn(users, top_n, ban_ptr, ban_item)
    assert t.counter(39) - before == S and not nan.any() and not want[3].any()
    np.testing.assert_array_equal(items, want[0])
    fe.same_bits_or_nan(scores, want[1], "rank_topn scores")
    np.testing.assert_array_equal(count, want[2])
    if not trained:   # the inputs are what the docstring says
        listed = want[1][want[0] >= 0]
        if stratum == "denormal":
            assert (np.abs(listed) < fe.FLT_MIN).all() and (listed != 0).any()
        else:
            assert ((np.diff(want[1], axis=1) == 0) & (want[0][:, 1:] >= 0) & (want[1][:, 1:] == 0)).sum() >= 12 * S
    # the lists fed back as positives hold the ranks 0, 1, 2, ..: both calls break ties the same way
    pos = [items[s, :count[s]].astype(np.uint32) for s in range(S)]
    pos_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    before = t.counter(38)
    position, tied, ranked, pnan = t.rank_positions(users, pos_ptr, np.concatenate(pos), ban_ptr, ban_item)
    assert t.counter(38) - before == S and not pnan.any()
    np.testing.assert_array_equal(position, np.concatenate([np.arange(n) for n in count]))
    t.close()

"""Hard negatives for passes of a pair source (svdf_*_pair_source*_hard) on the GPU: one kernel draws a pair's
candidates by the plain rule, scores them with the live model and keeps the best.

Expected columns: svdf_pair_hard_negatives on the trainer's own views (the host loop) and tests/pair_hard_rule.py (numpy, written from the
statement) -- ids equal, scores bit for bit (a NaN equal to any NaN), in both forms of the kernel (knob pair_hard_form 1 / 2).  Expected
models: a twin trainer started from the same model file, given the rule's column through dataset_from_pairs -- every view bit for bit.
Counters 44 / 45 tell the routes apart as in the plain pass; 46 counts the hard passes."""
import numpy as np
import pytest

import cases
import pair_hard_rule as hard
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu

NU, NI, N = hard.NU, hard.NI, hard.N
SHAPES = hard.SHAPES
C_HBM, C_FALLBACK, C_HARD = 44, 45, 46
VIEWS = ("W_user", "W_item", "i_bias")
MB = [("amd:step", "minibatch")]
FORMS = (1, 2)


def _trainer(k, extra=(), knobs=(), model=None, views=None):
    t = sa.Trainer(0, 3)
    t.seed(10)
    for key, v in cases.conf_with(cases.PAIR_CONF, num_user=NU, num_item=NI, num_factor=k) + list(extra):
        t.set_param(key, str(v))
    if model is None:
        t.init_model()
    else:
        t.load_model(model)
    t.init_trainer()
    for key, v in knobs:
        t.set_knob(key, v)
    if views is not None:
        for name, v in zip(VIEWS, views):
            t.set_view(name, v)
    return t


def _W(t):
    return [t.view(v) for v in VIEWS]


def _draw_both_forms(t, src, m, C, seed):
    """the column and the scores of a hard draw, equal in both forms of the kernel"""
    out = []
    for form in FORMS:
        t.set_knob("pair_hard_form", form)
        out.append(t.pair_source_draw(src, m, seed, hard=C, return_scores=True))
    t.set_knob("pair_hard_form", 0)
    neg = t.pair_source_draw(src, m, seed, hard=C)
    (n1, s1), (n2, s2) = out
    assert n1.dtype == np.uint32 and s1.dtype == np.float32 and n1.shape == s1.shape == (src.num_row * m,)
    assert np.array_equal(n1, n2) and hard.same_scores(s1, s2) and np.array_equal(neg, n1), "the two forms differ"
    return n1, s1


def _check(t, u, p, m, C, seed, numpy_too):
    src = t.pair_source(u, p)
    neg, score = _draw_both_forms(t, src, m, C, seed)
    src.close()
    W = _W(t)
    want = sa.pair_hard_negatives(NU, NI, u, p, m, C, seed, *W, return_scores=True)
    assert np.array_equal(neg, want[0]) and hard.same_scores(score, want[1]), "differs from svdf_pair_hard_negatives"
    if numpy_too:
        want = hard.rule_hard(NU, NI, u, p, m, C, seed, *W)
        assert np.array_equal(neg, want[0]) and hard.same_scores(score, want[1]), "differs from the numpy rule"
    return neg, score


@pytest.mark.parametrize("k", [1, 3, 4, 5, 16, 64, 128, 256, 257, 320])
def test_the_hard_column_is_the_rule_at_every_width(k):
    """tails 1 .. 3, the LDS width steps 64 / 128 / 256, the wide fallback (form 2 falls to 1); every (num_neg, num_cand) shape: num_cand not
    dividing 64, 64, above 64, 256"""
    t = _trainer(k, views=hard.model(k))
    for j, (m, C) in enumerate(SHAPES):
        for n in (65, N):
            u, p = hard.rows("grouped" if j % 2 else "shuffled", n)
            _check(t, u, p, m, C, 300 + n + j, numpy_too=n * m * C * max(k, 8) <= 50_000_000)   # (numpy: up to about 2 s a width)
    t.close()


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_the_hard_column_is_the_rule_at_every_size(order):
    """sources of one row, one wave's pairs less one, exactly, plus one, several waves with a ragged end"""
    t = _trainer(16, views=hard.model(16))
    for n in (1, 63, 64, 65, 257, N):
        u, p = hard.rows(order, n)
        for m, C in SHAPES:
            _check(t, u, p, m, C, 99 + n, numpy_too=n <= 257 or m * C <= 8)
    t.close()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """a model file per width, after one pass over planted pairs so that rows differ"""
    out = {}
    for k in (16, 64, 128):
        t = _trainer(k)
        ds = t.dataset_from_pairs(*cases.planted_pairs(2000, NU, NI, seed=3))
        t.train_dataset(ds)
        ds.close()
        out[k] = str(tmp_path_factory.mktemp("pair_hard") / ("model_%d" % k))
        t.save_model(out[k])
        t.close()
    return out


@pytest.mark.parametrize("m,C", [(1, 8), (2, 3), (1, 100)])
def test_the_negatives_of_the_candidate_call(models, m, C):
    """the parent's only route to these negatives: the plain draw with m * C negatives per row copied to the host, then rank_topn with top_n 1
    over one candidate list per pair -- on a trained model, where nothing ties"""
    t = _trainer(64, model=models[64])
    u, p = hard.rows("shuffled")
    src = t.pair_source(u, p)
    cand = t.pair_source_draw(src, m * C, 21)
    items, scores, count, nan = t.rank_topn(np.repeat(u, m), 1, candidates=(C * np.arange(N * m + 1, dtype=np.int64), cand))
    assert (count == 1).all() and not nan.any()
    untied = hard.rule_hard(NU, NI, u, p, m, C, 21, *_W(t), full=True)[4]
    assert untied.sum() > 0.99 * N * m
    neg, score = _draw_both_forms(t, src, m, C, 21)
    assert np.array_equal(neg[untied], items[untied, 0].astype(np.uint32))
    assert np.array_equal(neg, items[:, 0].astype(np.uint32))   # ... and a tie goes to the smaller id on both routes
    assert hard.same_scores(score, scores[:, 0])
    src.close()
    t.close()


def test_ties_zeros_nan_and_inf():
    u, p = hard.rows("shuffled")
    u[10:40], u[40:60] = 5, 7   # the users whose rows hold NaN in nan_model
    for W, m, C in ((hard.tie_model(), 1, 8), (hard.zero_model(), 2, 8), (hard.nan_model(), 1, 4), (hard.nan_model(), 1, 70), (hard.inf_model(), 1, 8)):
        t = _trainer(W[0].shape[1], views=W)
        neg, score = _check(t, u, p, m, C, 5, numpy_too=True)
        _, _, cand, sc, _ = hard.rule_hard(NU, NI, u, p, m, C, 5, *W, full=True)
        all_nan = np.isnan(sc).all(1)
        assert np.array_equal(neg[all_nan], cand[all_nan, 0]) and np.isnan(score[all_nan]).all() and not np.isnan(score[~all_nan]).any()
        t.close()
    assert all_nan.sum() == 0   # (the last model: +-inf are ordinary scores)


@pytest.mark.parametrize("k", [5, 16, 64, 128, 256])
def test_the_rounding_inputs(k):
    """inputs on which every other order of the same additions moves at least 20 of the 3 000 choices (tests/test_pair_hard.py asserts that
    on the CPU): the kernel's two forms give the pinned order's"""
    t = _trainer(k, views=hard.rounding_model(k))
    u, p = hard.rows("shuffled")
    _check(t, u, p, 1, 8, 11, numpy_too=True)
    t.close()


def test_a_hard_draw_follows_the_training_pass_on_the_stream(models):
    """train_dataset, then a hard draw WITHOUT a synchronize in between: the candidates are scored with the model the pass leaves"""
    t = _trainer(64, model=models[64])
    u, p = hard.rows("shuffled")
    src = t.pair_source(u, p)
    ds = t.dataset_from_pairs(*cases.planted_pairs(3000, NU, NI, seed=9))
    before = _W(t)
    for form in FORMS:
        t.set_knob("pair_hard_form", form)
        t.train_dataset(ds)
        neg, score = t.pair_source_draw(src, 1, 4, hard=8, return_scores=True)
        after = _W(t)
        want = hard.rule_hard(NU, NI, u, p, 1, 8, 4, *after)
        assert np.array_equal(neg, want[0]) and hard.same_scores(score, want[1])
        stale = hard.rule_hard(NU, NI, u, p, 1, 8, 4, *before)
        assert not hard.same_scores(score, stale[1])   # (the pass moved the scores)
        before = after
    src.close()
    t.close()


def _views(t):
    return [t.view(v).view(np.uint32).copy() for v in VIEWS]


def _twins(models, k, order, m, C, extra=(), knobs=(), rounds=2, seed=77):
    """(source trainer, twin, their data sets of the last round, counters moved) after `rounds` hard passes with seeds seed, seed + 1, ..: the
    twin trains dataset_from_pairs on the column the numpy rule gives on the model as it stands, so the second round's choice depends on the
    first round's training"""
    u, p = hard.rows(order)
    a, b = _trainer(k, extra, knobs, models[k]), _trainer(k, extra, knobs, models[k])
    src = a.pair_source(u, p)
    before = [a.counter(c) for c in (C_HBM, C_FALLBACK, C_HARD)]
    da = db = None
    for r in range(rounds):
        neg = hard.rule_hard(NU, NI, u, p, m, C, seed + r, *_W(b))[0]
        da = a.dataset_from_pair_source(src, m, seed + r, hard=C)
        db = b.dataset_from_pairs(np.repeat(u, m), np.repeat(p, m), neg)
        assert (da.kind, da.num_row, da.num_batches, da.info(8)) == (db.kind, db.num_row, db.num_batches, db.info(8))
        a.train_dataset(da)
        b.train_dataset(db)
    for x, y, name in zip(_views(a), _views(b), VIEWS):
        assert np.array_equal(x, y), "%s differs from the twin's" % name
    src.close()
    return a, b, da, db, tuple(a.counter(c) - x for c, x in zip((C_HBM, C_FALLBACK, C_HARD), before))


@pytest.mark.parametrize("k", [16, 64, 128])
def test_exact_hard_pass_stays_in_hbm(models, k):
    a, b, da, db, moved = _twins(models, k, "shuffled", 1, 8)
    assert moved == (2, 0, 2) and da.kind == 2
    assert np.array_equal(a.predict_dataset(da).view(np.uint32), b.predict_dataset(db).view(np.uint32))


def test_exact_hard_pass_with_three_negatives_per_row(models):
    *_, moved = _twins(models, 64, "shuffled", 3, 4)
    assert moved == (0, 2, 2)   # the expanded user column is user-grouped: user-run units are built on the host, as in the plain pass
    *_, moved = _twins(models, 64, "shuffled", 3, 4, knobs=[("pair_units", 0)])
    assert moved == (2, 0, 2)


def test_exact_hard_pass_of_a_user_grouped_source(models):
    a, b, da, db, moved = _twins(models, 64, "grouped", 1, 8)
    assert moved == (0, 2, 2) and da.kind == db.kind


@pytest.mark.parametrize("form", FORMS)
def test_window_step_hard_pass_stays_in_hbm(models, form):
    a, b, da, db, moved = _twins(models, 64, "shuffled", 1, 8, extra=MB + [("amd:window", 400)], knobs=[("pair_hard_form", form)])
    assert moved == (2, 0, 2)
    assert da.kind == 8 and da.info(8) == 5 and da.num_batches == db.num_batches > 1


def test_fallback_configuration(models):
    *_, moved = _twins(models, 64, "shuffled", 1, 8, extra=MB + [("amd:window", 400)], knobs=[("window_pair_sub", 16)])
    assert moved == (0, 2, 2)


def test_one_candidate_is_the_plain_pass(models):
    u, p = hard.rows("shuffled")
    a, b = _trainer(64, model=models[64]), _trainer(64, model=models[64])
    sa_, sb = a.pair_source(u, p), b.pair_source(u, p)
    for m in (1, 3):
        neg, score = _draw_both_forms(a, sa_, m, 1, 13)
        assert np.array_equal(neg, b.pair_source_draw(sb, m, 13)) and np.array_equal(neg, sa.pair_negatives(NU, NI, u, p, m, 13))
        assert hard.same_scores(score, hard.rule_hard(NU, NI, u, p, m, 1, 13, *_W(a))[1])
    da, db = a.dataset_from_pair_source(sa_, 1, 13, hard=1), b.dataset_from_pair_source(sb, 1, 13)
    assert (da.kind, da.num_row, da.num_batches, da.info(8)) == (db.kind, db.num_row, db.num_batches, db.info(8))
    a.train_dataset(da)
    b.train_dataset(db)
    assert all(np.array_equal(x, y) for x, y in zip(_views(a), _views(b)))
    assert (a.counter(C_HBM), a.counter(C_HARD), b.counter(C_HBM), b.counter(C_HARD)) == (1, 1, 1, 0)
    sa_.close()
    sb.close()


def test_lifetimes_and_a_second_trainers_source(models):
    u, p = hard.rows("shuffled")
    t, twin, other = _trainer(64, model=models[64]), _trainer(64, model=models[64]), _trainer(64, model=models[64])
    src = t.pair_source(u, p)
    ds = t.dataset_from_pair_source(src, 1, 3, hard=8)
    for call in (lambda: other.dataset_from_pair_source(src, 1, 3, hard=8), lambda: other.pair_source_draw(src, 1, 3, hard=8)):
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call()
    src.close()
    src.close()
    t.train_dataset(ds)   # the data set outlives its source
    dt = twin.dataset_from_pairs(u, p, hard.rule_hard(NU, NI, u, p, 1, 8, 3, *_W(twin))[0])
    twin.train_dataset(dt)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    assert other.counter(C_HBM) == other.counter(C_FALLBACK) == other.counter(C_HARD) == 0
    late = t.pair_source(u, p)
    t.close()
    with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
        other.pair_source_draw(late, 1, 3, hard=8)   # ... and the source of a trainer that is gone
    late.close()
    ds.close()

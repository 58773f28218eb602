"""Passes of rank pairs from positives only (svdf_pair_source_*): the device draws the negatives of a pass by the
published rule and builds the pass from the columns where they are.

Expected negatives: tests/pair_source_rule.py (numpy, written from the statement) and svdf_pair_negatives (the host loop).  Expected models:
a twin trainer started from the same model file, given the host rule's columns through dataset_from_pairs -- every view bit for bit.  The
routes are told apart by counters 44 (the pair columns stayed in HBM) and 45 (dataset_from_pairs on the columns copied back)."""
import numpy as np
import pytest

import cases
import pair_source_rule as rule
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu

NU, NI, N = 200, 300, 3000
C_HBM, C_FALLBACK = 44, 45
VIEWS = ("W_user", "W_item", "i_bias")
MB = [("amd:step", "minibatch")]


def _rows(order, n=N, seed=5):
    """n positives of 200 users x 300 items with repeated (user, item) rows; users 0 and 1 have no row, user 2 has one"""
    rng = np.random.default_rng(seed)
    u = rng.integers(3, NU, n)
    u[0] = 2
    p = rng.integers(0, NI, n)
    p[n // 2:n // 2 + min(20, n // 2)] = p[:min(20, n // 2)]
    u[n // 2:n // 2 + min(20, n // 2)] = u[:min(20, n // 2)]
    if order == "grouped":
        at = np.argsort(u, kind="stable")
        u, p = u[at], p[at]
    return u.astype(np.uint32), p.astype(np.uint32)


def _trainer(k, extra=(), knobs=(), model=None, nu=NU, ni=NI):
    t = sa.Trainer(0, 3)
    t.seed(10)
    for key, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k) + list(extra):
        t.set_param(key, str(v))
    if model is None:
        t.init_model()
    else:
        t.load_model(model)
    t.init_trainer()
    for key, v in knobs:
        t.set_knob(key, v)
    return t


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """a model file per width, after one pass over planted pairs so that rows differ"""
    out = {}
    for k in (16, 64, 128):
        t = _trainer(k)
        ds = t.dataset_from_pairs(*cases.planted_pairs(2000, NU, NI, seed=3))
        t.train_dataset(ds)
        ds.close()
        out[k] = str(tmp_path_factory.mktemp("pair_source") / ("model_%d" % k))
        t.save_model(out[k])
        t.close()
    return out


def _views(t):
    return [t.view(v).view(np.uint32).copy() for v in VIEWS]


def _twins(models, k, order, num_neg, extra=(), knobs=(), rounds=2, seed=77):
    """(source trainer, twin, their data sets of the last round, counters moved) after `rounds` passes with seeds seed, seed + 1, .."""
    u, p = _rows(order)
    a, b = _trainer(k, extra, knobs, models[k]), _trainer(k, extra, knobs, models[k])
    src = a.pair_source(u, p)
    before = (a.counter(C_HBM), a.counter(C_FALLBACK))
    da = db = None
    for r in range(rounds):
        neg = sa.pair_negatives(NU, NI, u, p, num_neg, seed + r)
        da = a.dataset_from_pair_source(src, num_neg, seed + r)
        db = b.dataset_from_pairs(np.repeat(u, num_neg), np.repeat(p, num_neg), neg)
        assert (da.kind, da.num_row, da.num_batches, da.info(8)) == (db.kind, db.num_row, db.num_batches, db.info(8))
        a.train_dataset(da)
        b.train_dataset(db)
    for x, y, name in zip(_views(a), _views(b), VIEWS):
        assert np.array_equal(x, y), "%s differs from the twin's" % name
    src.close()
    return a, b, da, db, (a.counter(C_HBM) - before[0], a.counter(C_FALLBACK) - before[1])


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_the_drawn_column_is_the_rule(order):
    t = _trainer(16)
    for n in (1, 63, 64, 65, 257, N):
        u, p = _rows(order, n)
        src = t.pair_source(u, p)
        for m in (1, 2, 5):
            got = t.pair_source_draw(src, m, 99 + n)
            assert got.dtype == np.uint32 and got.shape == (n * m,)
            assert np.array_equal(got, sa.pair_negatives(NU, NI, u, p, m, 99 + n))
            assert np.array_equal(got, rule.rule_negatives(NU, NI, u, p, m, 99 + n))
        src.close()
    t.close()


def test_the_pinned_rows_and_a_64_bit_seed():
    t = _trainer(16, nu=10, ni=1200)
    src = t.pair_source([4, 4, 9], [10, 700, 10])
    assert t.pair_source_draw(src, 1, 12345).tolist() == [607, 549, 766]
    assert t.pair_source_draw(src, 2, 12345).tolist() == [607, 549, 766, 1010, 64, 448]
    big = (1 << 63) + 12345
    assert np.array_equal(t.pair_source_draw(src, 3, big), rule.rule_negatives(10, 1200, [4, 4, 9], [10, 700, 10], 3, big))
    src.close()
    taken = t.pair_source([4, 4], [10, 607])
    assert t.pair_source_draw(taken, 1, 12345).tolist()[0] == 1083   # 607 is the user's: the second draw
    t.close()


def test_a_user_at_the_density_limit():
    """6 300 of 6 400 items are the user's: every draw is accepted with probability exactly 1 / 64"""
    ni = 6400
    u = np.concatenate([np.zeros(6300, np.uint32), np.ones(50, np.uint32)])
    p = np.concatenate([np.arange(6300), np.arange(50)]).astype(np.uint32)
    t = _trainer(16, nu=2, ni=ni)
    src = t.pair_source(u, p)
    got = t.pair_source_draw(src, 1, 7)
    want, took = rule.rule_negatives(2, ni, u, p, 1, 7, return_draws=True)
    assert np.array_equal(got, want) and (got[:6300] >= 6300).all() and took.max() < rule.T
    with pytest.raises(sa.SvdfError, match="pair_source: user 0 has 6301 distinct positive items of 6400"):
        t.pair_source(np.zeros(6301, np.uint32), np.arange(6301, dtype=np.uint32))
    t.close()


@pytest.mark.parametrize("k", [16, 64, 128])
def test_exact_pass_of_a_shuffled_source_stays_in_hbm(models, k):
    a, b, da, db, moved = _twins(models, k, "shuffled", 1)
    assert moved == (2, 0) and da.kind == 2
    # the data sets score alike too
    assert np.array_equal(a.predict_dataset(da).view(np.uint32), b.predict_dataset(db).view(np.uint32))
    assert a.eval_dataset(da) == b.eval_dataset(db)


def test_exact_pass_with_three_negatives_per_row(models):
    """the three pairs of a row are adjacent, so the expanded user column is user-grouped: dataset_from_pairs' own pretest sends it to
    user-run units, which are built on the host; with that walker off the pass is scheduled in HBM"""
    *_, moved = _twins(models, 64, "shuffled", 3)
    assert moved == (0, 2)
    *_, moved = _twins(models, 64, "shuffled", 3, knobs=[("pair_units", 0)])
    assert moved == (2, 0)


def test_exact_pass_of_a_user_grouped_source_takes_the_fallback(models):
    a, b, da, db, moved = _twins(models, 64, "grouped", 1)
    assert moved == (0, 2) and da.kind == db.kind


@pytest.mark.parametrize("k,num_neg", [(16, 1), (64, 2), (128, 1)])
def test_window_step_stays_in_hbm(models, k, num_neg):
    a, b, da, db, moved = _twins(models, k, "shuffled", num_neg, extra=MB + [("amd:window", 400)])
    assert moved == (2, 0)
    assert da.kind == 8 and da.info(8) == 5 and da.num_batches == db.num_batches > 1
    assert np.array_equal(a.predict_dataset(da).view(np.uint32), b.predict_dataset(db).view(np.uint32))
    assert a.eval_dataset(da) == b.eval_dataset(db)


def test_window_step_with_the_rule_deciding_the_windows(models):
    a, b, da, db, moved = _twins(models, 64, "grouped", 1, extra=MB)
    assert moved == (2, 0) and da.info(8) == 5


def test_fallback_configurations(models, tmp_path):
    *_, moved = _twins(models, 64, "shuffled", 1, extra=MB + [("amd:window", 400)], knobs=[("window_pair_sub", 16)])
    assert moved == (0, 2)
    table = tmp_path / "fi.txt"
    table.write_text("".join("1 %d:0.5\n" % ((i * 7) % NI) if i % 3 == 0 else "0\n" for i in range(NI)))
    *_, moved = _twins(models, 16, "shuffled", 2, extra=[("feature_item", str(table))], rounds=1)
    assert moved == (0, 1)


def test_lifetimes(models):
    u, p = _rows("shuffled")
    t, twin = _trainer(64, model=models[64]), _trainer(64, model=models[64])
    src = t.pair_source(u, p)
    ds = t.dataset_from_pair_source(src, 1, 3)
    src.close()
    src.close()
    t.train_dataset(ds)   # the data set outlives its source
    dt = twin.dataset_from_pairs(u, p, sa.pair_negatives(NU, NI, u, p, 1, 3))
    twin.train_dataset(dt)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    late = t.pair_source(u, p)
    t.close()
    late.close()          # after the trainer
    ds.close()


def test_dataset_from_pairs_is_untouched_by_the_source_calls(models):
    u, p, q = cases.planted_pairs(1500, NU, NI, seed=8)
    t, twin = _trainer(64, model=models[64]), _trainer(64, model=models[64])
    fixed, fixed_twin = t.dataset_from_pairs(u, p, q), twin.dataset_from_pairs(u, p, q)
    t.train_dataset(fixed)
    twin.train_dataset(fixed_twin)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    src = t.pair_source(*_rows("shuffled"))
    t.pair_source_draw(src, 2, 1)
    t.dataset_from_pair_source(src, 1, 1).close()   # built, not trained
    again, again_twin = t.dataset_from_pairs(u, p, q), twin.dataset_from_pairs(u, p, q)
    t.train_dataset(again)
    twin.train_dataset(again_twin)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    assert (again.kind, again.num_batches) == (again_twin.kind, again_twin.num_batches)


def test_a_second_trainers_source_is_refused():
    a, b = _trainer(16), _trainer(16)
    src = a.pair_source(*_rows("shuffled", 65))
    for call in (lambda: b.dataset_from_pair_source(src, 1, 1), lambda: b.pair_source_draw(src, 1, 1)):
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call()
    a.close()
    with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
        b.pair_source_draw(src, 1, 1)   # ... and the source of a trainer that is gone
    assert b.counter(C_HBM) == b.counter(C_FALLBACK) == 0

"""Shuffled passes of the pair source on the device (svdf_dataset_from_pair_source_shuffled / svdf_pair_source_draw_shuffled, DESIGN.md
section 6af): k_pair_order gathers the rows in the order sigma before the unchanged draw kernels, and counts the adjacent positions that
share a user for the route decision.

Expected columns: tests/pair_order_rule.py (numpy, written from the statement) and the host rules on the permuted rows.  Expected models and
routes: a TWIN trainer started from the same model file whose source is created from the host-permuted rows and trained with the unshuffled
call -- every view bit for bit, counters 44 / 45 moved as the twin's; counter 48 counts the shuffled passes."""
import numpy as np
import pytest

import cases
import pair_order_rule as rule
import pair_weight_rule
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu

NU, NI = rule.NU, rule.NI
C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED, C_SHUFFLED = 44, 45, 46, 47, 48
COUNTERS = (C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED, C_SHUFFLED)
VIEWS = ("W_user", "W_item", "i_bias")
MB = [("amd:step", "minibatch"), ("amd:window", 400)]


def _trainer(k, extra=(), knobs=(), model=None):
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
    return t


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """a model file per width, after one pass over planted pairs so that rows differ"""
    out = {}
    for k in (16, 128):
        t = _trainer(k)
        ds = t.dataset_from_pairs(*cases.planted_pairs(2000, NU, NI, seed=3))
        t.train_dataset(ds)
        ds.close()
        out[k] = str(tmp_path_factory.mktemp("pair_order") / ("model_%d" % k))
        t.save_model(out[k])
        t.close()
    return out


def _views(t):
    return [t.view(v).view(np.uint32).copy() for v in VIEWS]


def _weights():
    w = 1 + (np.arange(NI, dtype=np.int64) * 37) % 11
    w[::13] = 0
    return w.astype(np.uint32)


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_the_drawn_columns_are_the_rule(order):
    """the wave and block edges of k_pair_order: 1, 2, 3 rows, 63 / 64 / 65, 255 / 256 / 257, and 3 000"""
    t = _trainer(16)
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 3000):
        u, p = rule.rows(order, n)
        src = t.pair_source(u, p)
        for m in (1, 3):
            for s in (n, (1 << 64) - 1 - n):
                sigma = rule.sigma(n, s).astype(np.int64)
                got = t.pair_source_draw(src, m, 99 + n, shuffle=s)
                assert len(got) == 3 and all(c.dtype == np.uint32 and c.shape == (n * m,) for c in got)
                assert np.array_equal(got[0], np.repeat(u[sigma], m)) and np.array_equal(got[1], np.repeat(p[sigma], m)), (n, m, s)
                assert np.array_equal(got[2], sa.pair_negatives(NU, NI, u[sigma], p[sigma], m, 99 + n)), (n, m, s)
        src.close()
    t.close()


def test_the_pinned_pass():
    t = _trainer(16)
    src = t.pair_source([4, 4, 9], [10, 700, 10])
    got = t.pair_source_draw(src, 1, 12345, shuffle=12345)
    assert list(zip(*[c.tolist() for c in got])) == [(4, 700, 607), (9, 10, 549), (4, 10, 766)]
    src.close()
    t.close()


def _twins(models, k, rows, m, C=None, extra=(), knobs=(), shuffles=(5, 6), seed=77, weights=None):
    """(source trainer, twin, their data sets of the last round, what counters 44 .. 48 moved by on each) after one pass per entry of `shuffles`
    (None: the unshuffled call on both): the twin's source holds the host-permuted rows and takes the unshuffled call"""
    u, p = rows
    a, b = _trainer(k, extra, knobs, models[k]), _trainer(k, extra, knobs, models[k])
    src = a.pair_source(u, p, item_weight=weights)
    before = [[x.counter(c) for c in COUNTERS] for x in (a, b)]
    da = db = None
    for r, s in enumerate(shuffles):
        sigma = np.arange(len(u)) if s is None else sa.pair_order(len(u), s).astype(np.int64)
        twin_src = b.pair_source(u[sigma], p[sigma], item_weight=weights)
        if C is not None:   # the chosen candidates and their scores, on models that are still equal
            ga = a.pair_source_draw(src, m, seed + r, hard=C, return_scores=True, shuffle=s)
            gb = b.pair_source_draw(twin_src, m, seed + r, hard=C, return_scores=True)
            assert np.array_equal(ga[-2], gb[0]) and np.array_equal(ga[-1].view(np.uint32), gb[1].view(np.uint32))
        da = a.dataset_from_pair_source(src, m, seed + r, hard=C, shuffle=s)
        db = b.dataset_from_pair_source(twin_src, m, seed + r, hard=C)
        twin_src.close()
        assert (da.kind, da.num_row, da.num_batches, da.info(8)) == (db.kind, db.num_row, db.num_batches, db.info(8))
        a.train_dataset(da)
        b.train_dataset(db)
    for x, y, name in zip(_views(a), _views(b), VIEWS):
        assert np.array_equal(x, y), "%s differs from the twin's" % name
    src.close()
    moved = [tuple(x.counter(c) - y for c, y in zip(COUNTERS, was)) for x, was in zip((a, b), before)]
    assert moved[0][:4] == moved[1][:4], "the routes differ from the twin's"
    assert moved[1][4] == 0 and moved[0][4] == sum(s is not None for s in shuffles)
    return a, b, da, db, moved[0]


@pytest.mark.parametrize("k", [16, 128])
@pytest.mark.parametrize("m", [1, 3])
def test_exact_pass(models, k, m):
    a, b, da, db, moved = _twins(models, k, rule.rows("shuffled"), m)
    assert moved == ((2, 0, 0, 0, 2) if m == 1 else (0, 2, 0, 0, 2)) and da.kind == db.kind
    a.close()
    b.close()


def test_three_negatives_stay_in_hbm_without_pair_units(models):
    *_, moved = _twins(models, 16, rule.rows("shuffled"), 3, knobs=[("pair_units", 0)])
    assert moved == (2, 0, 0, 0, 2)


def test_hard_pass(models):
    *_, moved = _twins(models, 128, rule.rows("shuffled"), 1, C=4)
    assert moved == (2, 0, 2, 0, 2)
    *_, moved = _twins(models, 16, rule.rows("grouped"), 3, C=4)
    assert moved == (0, 2, 2, 0, 2)


def test_weighted_source(models):
    *_, moved = _twins(models, 16, rule.rows("shuffled"), 1, weights=_weights())
    assert moved == (2, 0, 0, 2, 2)
    *_, moved = _twins(models, 16, rule.rows("grouped"), 1, C=2, weights=_weights())
    assert moved == (2, 0, 2, 2, 2)


def test_window_step(models):
    a, b, da, db, moved = _twins(models, 128, rule.rows("grouped"), 1, extra=MB)
    assert moved == (2, 0, 0, 0, 2)
    assert da.kind == 8 and da.num_batches == db.num_batches > 1 and da.info(8) == db.info(8)


def test_a_user_grouped_source_stays_in_hbm_when_shuffled(models):
    rows = rule.rows("grouped")
    assert 2 * rule.same(rows[0], np.arange(3000)) >= 3000
    *_, moved = _twins(models, 16, rows, 1, shuffles=(None, None))
    assert moved == (0, 2, 0, 0, 0)        # unshuffled: user-run units through the fallback
    *_, moved = _twins(models, 16, rows, 1, shuffles=(5, 6))
    assert moved == (2, 0, 0, 0, 2)        # shuffled: the exact pass from the columns in HBM
    *_, moved = _twins(models, 16, rows, 1, shuffles=(5, None, 7))
    assert moved == (2, 1, 0, 0, 2)


def test_one_users_rows_stay_grouped(models):
    n = 200
    u = np.full(n, 7, np.uint32)
    p = np.random.default_rng(1).integers(0, NI, n).astype(np.uint32)
    *_, moved = _twins(models, 16, (u, p), 1)
    assert moved == (0, 2, 0, 0, 2)


@pytest.mark.parametrize("n,drop", [(258, None), (258, 64), (258, 128), (258, 192), (258, 256), (258, 1), (258, 257), (130, None), (130, 64)])
def test_the_adjacent_count_at_wave_and_block_edges(models, n, drop):
    """rows placed so that, in the PERMUTED order, exactly n / 2 positions share their user with the one before -- the first lanes of the waves
    (64, 128, 192) and of the second block (256) among them: 2 * same == n is the user-run route (45).  With any one of them dropped
    2 * same < n and the pass stays in HBM (44).  A device count that misses or double-counts an edge takes the other route."""
    s = 31
    sigma = sa.pair_order(n, s).astype(np.int64)
    edges = [e for e in (1, 64, 128, 192, 256, n - 1) if e < n]
    rest = [q for q in range(2, n - 1) if q not in edges]
    positions = set(edges + rest[:n // 2 - len(edges)])
    positions.discard(drop)
    assert len(positions) == n // 2 - (drop is not None)
    u, p = rule.rows_with_same_at(n, sigma, positions)
    assert rule.same(u, sigma) == len(positions)
    *_, moved = _twins(models, 16, (u, p), 1, shuffles=(s,))
    assert moved == ((0, 1, 0, 0, 1) if drop is None else (1, 0, 0, 0, 1))


def test_none_is_the_old_call(models):
    u, p = rule.rows("shuffled")
    t = _trainer(16, model=models[16])
    src = t.pair_source(u, p)
    for m in (1, 3):
        old = sa.pair_negatives(NU, NI, u, p, m, 9)
        assert np.array_equal(t.pair_source_draw(src, m, 9), old) and np.array_equal(t.pair_source_draw(src, m, 9, shuffle=None), old)
        h = t.pair_source_draw(src, m, 9, hard=2, return_scores=True)
        g = t.pair_source_draw(src, m, 9, hard=2, return_scores=True, shuffle=None)
        assert len(g) == 2 and np.array_equal(h[0], g[0]) and np.array_equal(h[1].view(np.uint32), g[1].view(np.uint32))
    assert [t.counter(c) for c in COUNTERS] == [0, 0, 0, 0, 0]   # a draw is not a pass
    t.dataset_from_pair_source(src, 1, 1).close()
    t.dataset_from_pair_source(src, 1, 1, shuffle=None).close()
    t.dataset_from_pair_source(src, 1, 1, hard=2, shuffle=None).close()
    assert [t.counter(c) for c in COUNTERS] == [3, 0, 1, 0, 0]
    t.dataset_from_pair_source(src, 1, 1, shuffle=0).close()        # an order_seed of 0 is an order
    t.dataset_from_pair_source(src, 1, 1, hard=2, shuffle=1).close()
    t.pair_source_draw(src, 1, 1, shuffle=2)
    assert [t.counter(c) for c in COUNTERS] == [5, 0, 2, 0, 2]
    # hard=1 equals plain on the shuffled pass too
    assert all(np.array_equal(x, y) for x, y in zip(t.pair_source_draw(src, 2, 4, shuffle=8), t.pair_source_draw(src, 2, 4, hard=1, shuffle=8)))
    src.close()
    t.close()


def test_lifetimes(models):
    u, p = rule.rows("grouped")
    t, twin = _trainer(128, model=models[128]), _trainer(128, model=models[128])
    src = t.pair_source(u, p)
    ds = t.dataset_from_pair_source(src, 1, 3, shuffle=4)
    src.close()
    src.close()
    t.train_dataset(ds)   # the data set outlives its source and the scratch columns of its pass
    sigma = sa.pair_order(len(u), 4).astype(np.int64)
    dt = twin.dataset_from_pairs(u[sigma], p[sigma], sa.pair_negatives(NU, NI, u[sigma], p[sigma], 1, 3))
    twin.train_dataset(dt)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    late = t.pair_source(u, p)
    other = _trainer(16)
    with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
        other.dataset_from_pair_source(late, 1, 1, shuffle=1)
    t.close()
    with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
        other.pair_source_draw(late, 1, 1, shuffle=1)   # ... and the source of a trainer that is gone
    late.close()          # after the trainer
    ds.close()
    other.close()
    twin.close()

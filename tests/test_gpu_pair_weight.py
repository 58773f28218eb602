"""Item-weighted negatives for the pair source on the device (svdf_pair_source_create_weighted): plain and hard passes
of a weighted source draw through its weight table, in both forms of the map (knob pair_weight_form 1 / 2) with equal bits.

Expected negatives: tests/pair_weight_rule.py (numpy / Python integers, written from the statement) and svdf_pair_negatives_weighted /
svdf_pair_hard_negatives_weighted (the host loops).  Expected models: a twin trainer started from the same model file, given the rule's
column through dataset_from_pairs -- every view bit for bit.  Counters 44 / 45 / 46 tell routes and hard passes apart as before; 47 counts
the passes drawn from a weighted source."""
import numpy as np
import pytest

import cases
import pair_hard_rule as hard
import pair_weight_rule as rule
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu

NU, NI, N = rule.NU, rule.NI, rule.N
C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED = 44, 45, 46, 47
VIEWS = ("W_user", "W_item", "i_bias")
MB = [("amd:step", "minibatch")]
ROW_TABLES = rule.row_tables()
TABLES = rule.tables()


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
    for k in (1, 5, 16, 64, 128, 257):
        t = _trainer(k)
        ds = t.dataset_from_pairs(*cases.planted_pairs(2000, NU, NI, seed=3))
        t.train_dataset(ds)
        ds.close()
        out[k] = str(tmp_path_factory.mktemp("pair_weight") / ("model_%d" % k))
        t.save_model(out[k])
        t.close()
    return out


def _views(t):
    return [t.view(v).view(np.uint32).copy() for v in VIEWS]


def _W(t):
    return [t.view(v) for v in VIEWS]


def _draw_all_forms(t, src, m, seed):
    """the plain column in forms 1, 2 and 0: equal bits"""
    out = []
    for form in (1, 2, 0):
        t.set_knob("pair_weight_form", form)
        out.append(t.pair_source_draw(src, m, seed))
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]), "the forms of the map differ"
    return out[0]


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("table", sorted(ROW_TABLES))
def test_the_drawn_column_is_the_rule(order, table):
    w = ROW_TABLES[table]
    t = _trainer(16)
    for n in (1, 63, 64, 65, 257, N):
        u, p = rule.rows(order, n)
        src = t.pair_source(u, p, item_weight=w)
        for m in (1, 2, 7, 256):
            got = _draw_all_forms(t, src, m, 99 + n)
            assert got.dtype == np.uint32 and got.shape == (n * m,)
            assert np.array_equal(got, sa.pair_negatives(NU, NI, u, p, m, 99 + n, item_weight=w)), (n, m)
            assert np.array_equal(got, rule.rule_negatives(NU, NI, u, p, w, m, 99 + n)), (n, m)
            assert (w[got] > 0).all()
        src.close()
    t.close()


@pytest.mark.parametrize("name", sorted(TABLES))
def test_every_table_probe_and_column(name):
    """each table of the lookup tests at its own catalogue size: the device probe on every boundary word, and -- where the table admits the
    rows -- the column of a small source"""
    w = TABLES[name]
    ni = len(w)
    cdf = rule.cdf_of(w)
    t = _trainer(16, ni=ni)
    x = rule.boundary_words(cdf)
    want = rule.lookups(cdf, x)
    for form in (1, 2, 0):
        got = sa.pair_weight_lookup(w, x, form, trainer=t)
        assert np.array_equal(got, want) and np.array_equal(got, sa.pair_weight_lookup(w, x, max(form, 1))), form
    u, p = rule.rows("shuffled", 257)
    p = (p % ni).astype(np.uint32)
    refusal = rule.density_refusal(NU, u, p, w)
    if refusal is not None:
        with pytest.raises(sa.SvdfError, match="pair_source: user %d's positive items hold %d of the total item weight %d" % refusal):
            t.pair_source(u, p, item_weight=w)
    else:
        src = t.pair_source(u, p, item_weight=w)
        for m in (1, 7):
            got = _draw_all_forms(t, src, m, 5)
            assert np.array_equal(got, sa.pair_negatives(NU, ni, u, p, m, 5, item_weight=w))
            assert np.array_equal(got, rule.rule_negatives(NU, ni, u, p, w, m, 5)) and (w[got] > 0).all()
        src.close()
    t.close()


@pytest.mark.parametrize("ni", [10000, 10001])
def test_the_measured_form_on_both_sides_of_its_threshold(ni):
    """pair_weight_form = 0 takes the guided search up to 10 000 items and the search of the whole table above: equal ids either way"""
    w = rule.pinned_weights(ni)
    cdf = rule.cdf_of(w)
    t = _trainer(16, nu=50, ni=ni)
    x = rule.boundary_words(cdf)
    want = rule.lookups(cdf, x)
    assert np.array_equal(sa.pair_weight_lookup(w, x, 0, trainer=t), want) and np.array_equal(sa.pair_weight_lookup(w, x, 0), want)
    u, p = np.arange(2000, dtype=np.uint32) % 50, (np.arange(2000, dtype=np.uint32) * 7) % ni
    src = t.pair_source(u, p, item_weight=w)
    assert np.array_equal(_draw_all_forms(t, src, 3, 11), rule.rule_negatives(50, ni, u, p, w, 3, 11))
    src.close()
    t.close()


def test_the_pinned_rows_beside_an_unweighted_source():
    """a weighted and an unweighted source of one trainer alive together: each keeps its own rule"""
    t = _trainer(16, nu=10, ni=1200)
    w = rule.pinned_weights()
    weighted, plain = t.pair_source([4, 4, 9], [10, 700, 10], item_weight=w), t.pair_source([4, 4, 9], [10, 700, 10])
    for form in (1, 2, 0):
        t.set_knob("pair_weight_form", form)
        assert t.pair_source_draw(weighted, 1, 12345).tolist() == [611, 547, 755]
        assert t.pair_source_draw(plain, 1, 12345).tolist() == [607, 549, 766]
        assert t.pair_source_draw(weighted, 2, 12345).tolist() == [611, 547, 755, 1006, 59, 447]
        assert t.pair_source_draw(plain, 2, 12345).tolist() == [607, 549, 766, 1010, 64, 448]
    big = (1 << 63) + 12345
    assert np.array_equal(t.pair_source_draw(weighted, 3, big), rule.rule_negatives(10, 1200, [4, 4, 9], [10, 700, 10], w, 3, big))
    none = t.pair_source([4, 4, 9], [10, 700, 10], item_weight=None)   # None is the old call
    assert t.pair_source_draw(none, 1, 12345).tolist() == [607, 549, 766]
    # a hard pass on each, scores growing with the id: the pinned candidates of num_neg 2
    for name, v in zip(VIEWS, (np.zeros((10, 16), np.float32), np.zeros((1200, 16), np.float32), np.arange(1200, dtype=np.float32))):
        t.set_view(name, v)
    assert t.pair_source_draw(weighted, 1, 12345, hard=2).tolist() == [611, 1006, 447]
    assert t.pair_source_draw(plain, 1, 12345, hard=2).tolist() == [607, 1010, 448]
    weighted.close()
    assert t.pair_source_draw(plain, 1, 12345).tolist() == [607, 549, 766]
    t.close()


def test_a_user_at_the_weighted_density_limit():
    """the user of items 0 .. 126 holds 6 300 of W = 6 400: every draw is accepted with probability exactly 1 / 64, and the count rule would
    refuse the rows"""
    w = np.ones(128, np.uint32)
    w[0], w[127] = 6300 - 126, 100
    u = np.concatenate([np.zeros(127, np.uint32), np.ones(50, np.uint32)])
    p = np.concatenate([np.arange(127), np.arange(50)]).astype(np.uint32)
    t = _trainer(16, nu=2, ni=128)
    src = t.pair_source(u, p, item_weight=w)
    got = _draw_all_forms(t, src, 50, 7)
    assert np.array_equal(got, rule.rule_negatives(2, 128, u, p, w, 50, 7)) and (got[:127 * 50] == 127).all()
    with pytest.raises(sa.SvdfError, match="pair_source: user 0 has 127 distinct positive items of 128"):
        t.pair_source(u, p)
    w[127] = 99
    with pytest.raises(sa.SvdfError, match="pair_source: user 0's positive items hold 6300 of the total item weight 6399"):
        t.pair_source(u, p, item_weight=w)
    t.close()


@pytest.mark.parametrize("k", [1, 5, 16, 64, 128, 257])
def test_hard_passes_in_every_pair_of_forms(models, k):
    u, p = rule.rows("shuffled", 600)
    w = ROW_TABLES["rows_300"]
    t = _trainer(k, model=models[k])
    src = t.pair_source(u, p, item_weight=w)
    model = _W(t)
    for m, C in ((1, 1), (1, 2), (1, 8), (3, 4), (1, 65)):
        want = sa.pair_hard_negatives(NU, NI, u, p, m, C, 31, *model, return_scores=True, item_weight=w)
        if k in (5, 64):
            cand = rule.rule_negatives(NU, NI, u, p, w, m * C, 31).astype(np.int64).reshape(-1, C)
            neg, score, _ = hard.select(cand, hard.scores(cand, u, m, *model))
            assert np.array_equal(want[0], neg) and hard.same_scores(want[1], score), "the host loop differs from the numpy rule"
        for hf in (1, 2):
            for wf in (1, 2):
                t.set_knob("pair_hard_form", hf)
                t.set_knob("pair_weight_form", wf)
                neg, score = t.pair_source_draw(src, m, 31, hard=C, return_scores=True)
                assert np.array_equal(neg, want[0]) and hard.same_scores(score, want[1]), (m, C, hf, wf)
        t.set_knob("pair_hard_form", 0)
        t.set_knob("pair_weight_form", 0)
        assert np.array_equal(t.pair_source_draw(src, m, 31, hard=C), want[0])
        if C == 1:
            assert np.array_equal(want[0], t.pair_source_draw(src, m, 31))   # hard=1 is the weighted plain pass
    src.close()
    t.close()


def _twins(models, k, order, m, C=None, extra=(), knobs=(), rounds=2, seed=77, table="rows_300"):
    """(source trainer, twin, their data sets of the last round, counters moved) after `rounds` passes of a weighted source with seeds seed,
    seed + 1, ..: the twin trains dataset_from_pairs on the host rule's column (a hard pass: on the twin's model as it stands)"""
    u, p = rule.rows(order)
    w = ROW_TABLES[table]
    a, b = _trainer(k, extra, knobs, models[k]), _trainer(k, extra, knobs, models[k])
    src = a.pair_source(u, p, item_weight=w)
    counters = (C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED)
    before = [a.counter(c) for c in counters]
    da = db = None
    for r in range(rounds):
        if C is None:
            neg = rule.rule_negatives(NU, NI, u, p, w, m, seed + r)
        else:
            neg = sa.pair_hard_negatives(NU, NI, u, p, m, C, seed + r, *_W(b), item_weight=w)
        da = a.dataset_from_pair_source(src, m, seed + r, hard=C)
        db = b.dataset_from_pairs(np.repeat(u, m), np.repeat(p, m), neg)
        assert (da.kind, da.num_row, da.num_batches, da.info(8)) == (db.kind, db.num_row, db.num_batches, db.info(8))
        a.train_dataset(da)
        b.train_dataset(db)
    for x, y, name in zip(_views(a), _views(b), VIEWS):
        assert np.array_equal(x, y), "%s differs from the twin's" % name
    src.close()
    assert [b.counter(c) for c in counters] == [0, 0, 0, 0]
    return a, b, da, db, tuple(a.counter(c) - x for c, x in zip(counters, before))


@pytest.mark.parametrize("k,form", [(16, 1), (64, 2), (64, 0)])
def test_exact_pass_of_a_shuffled_weighted_source_stays_in_hbm(models, k, form):
    a, b, da, db, moved = _twins(models, k, "shuffled", 1, knobs=[("pair_weight_form", form)])
    assert moved == (2, 0, 0, 2) and da.kind == 2


def test_window_step_of_a_weighted_source(models):
    a, b, da, db, moved = _twins(models, 64, "shuffled", 1, extra=MB + [("amd:window", 400)], table="heavy_thirds")
    assert moved == (2, 0, 0, 2)
    assert da.kind == 8 and da.info(8) == 5 and da.num_batches == db.num_batches > 1


def test_three_negatives_per_row(models):
    *_, moved = _twins(models, 64, "shuffled", 3)
    assert moved == (0, 2, 0, 2)
    *_, moved = _twins(models, 16, "shuffled", 3, knobs=[("pair_units", 0), ("pair_weight_form", 2)])
    assert moved == (2, 0, 0, 2)


def test_hard_pass_of_a_weighted_source(models):
    *_, moved = _twins(models, 64, "shuffled", 1, C=4)
    assert moved == (2, 0, 2, 2)
    *_, moved = _twins(models, 16, "shuffled", 1, C=4, extra=MB + [("amd:window", 400)], knobs=[("pair_weight_form", 2)])
    assert moved == (2, 0, 2, 2)


def test_a_user_grouped_weighted_source_takes_the_fallback(models):
    a, b, da, db, moved = _twins(models, 64, "grouped", 1)
    assert moved == (0, 2, 0, 2) and da.kind == db.kind


def test_counters_tell_weighted_from_unweighted_passes(models):
    u, p = rule.rows("shuffled")
    t = _trainer(16, model=models[16])
    weighted, plain = t.pair_source(u, p, item_weight=ROW_TABLES["ones_300"]), t.pair_source(u, p)
    t.dataset_from_pair_source(plain, 1, 1).close()
    assert [t.counter(c) for c in (C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED)] == [1, 0, 0, 0]
    t.dataset_from_pair_source(weighted, 1, 1).close()
    t.dataset_from_pair_source(weighted, 1, 1, hard=2).close()
    t.dataset_from_pair_source(plain, 1, 1, hard=2).close()
    assert [t.counter(c) for c in (C_HBM, C_FALLBACK, C_HARD, C_WEIGHTED)] == [4, 0, 2, 2]
    t.pair_source_draw(weighted, 2, 1)   # a draw is not a pass
    assert t.counter(C_WEIGHTED) == 2
    t.close()


def test_lifetimes(models):
    u, p = rule.rows("shuffled")
    w = ROW_TABLES["rows_300"]
    t, twin = _trainer(64, model=models[64]), _trainer(64, model=models[64])
    src = t.pair_source(u, p, item_weight=w)
    ds = t.dataset_from_pair_source(src, 1, 3)
    src.close()
    src.close()
    t.train_dataset(ds)   # the data set outlives its source and the source's tables
    dt = twin.dataset_from_pairs(u, p, sa.pair_negatives(NU, NI, u, p, 1, 3, item_weight=w))
    twin.train_dataset(dt)
    assert all(np.array_equal(x, y) for x, y in zip(_views(t), _views(twin)))
    late = t.pair_source(u, p, item_weight=w)
    t.close()
    late.close()          # after the trainer
    ds.close()


def test_a_second_trainers_weighted_source_is_refused():
    a, b = _trainer(16), _trainer(16)
    src = a.pair_source(*rule.rows("shuffled", 65), item_weight=ROW_TABLES["rows_300"])
    for call in (lambda: b.dataset_from_pair_source(src, 1, 1), lambda: b.pair_source_draw(src, 1, 1), lambda: b.pair_source_draw(src, 1, 1, hard=2)):
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call()
    a.close()
    with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
        b.pair_source_draw(src, 1, 1)   # ... and the source of a trainer that is gone
    assert b.counter(C_HBM) == b.counter(C_FALLBACK) == b.counter(C_WEIGHTED) == 0
    b.close()


def test_the_refusals_on_a_device_handle():
    t = _trainer(16, nu=20, ni=30)
    zero, big = np.zeros(30, np.uint32), np.zeros(30, np.uint32)
    big[[0, 1]] = 1 << 31
    with pytest.raises(sa.SvdfError, match="pair_source: the item weights sum to 0"):
        t.pair_source([1, 2], [2, 3], item_weight=zero)
    with pytest.raises(sa.SvdfError, match=r"pair_source: the item weights sum to 4294967296: the sum must stay below 2\^32"):
        t.pair_source([1, 2], [2, 3], item_weight=big)
    with pytest.raises(sa.SvdfError, match="pair_source: the item weights sum to 0"):
        sa.pair_weight_lookup(zero, [0], 1, trainer=t)
    t.close()

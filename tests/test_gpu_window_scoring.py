"""svdf_predict_dataset / svdf_eval_dataset on window data sets: the one-GPU window sequence of `amd:step = minibatch` /
`auto` (kind 8) and stand-alone windows (kinds 5 and 7).  Predictions come back in FILE order -- the order of the rows as they were handed to
svdf_dataset_from_* / svdf_dataset_window_from_* -- and equal, bit for bit, what the pinned C port of the reference (oracle.oracle: predict_batch,
predict_block = the reference's pred, apex_svd_base.h:445-454, and SVDPPFeature::predict, :583-591) gives for the same rows on the same model:
the engine's parameters are copied into the port through view / set_view after training.  With side tables the port loads the same table files
(tests/window_sim.py does the same for the training checker).

Every case also checks the evaluator: count == n and |ss - sum_float64 (p - label)^2| <= 1e-9 ss with p the file-order predictions (the bound
tests/test_gpu_native_multi.py uses for this evaluator: per-workgroup fp64 partial sums, long double on the host); rank pairs carry label 1
(apex_svd_data.cpp:905-911).  The difference p - label is formed in fp32, as RMSEEvaluator forms it (svd_feature_infer.cpp:43-47; k_sqerr_partials
keeps that), and squared and summed in float64.  Forming the difference in float64 instead is another quantity: it differs from the evaluator's by
the fp32 rounding of each difference (up to 2^-23 per term; measured 1.5e-9 of ss on the 0 / 1 labels of the k = 10 logistic case, where p - 1
rounds), which is why tests/test_gpu_native_multi.py compares that form at 1e-6.  That form is asserted as well, at the bound the formats give:
every fp32 difference is within 2^-24 relative of the exact one, its square within 2^-23, and all terms are positive, so the sums agree to
2^-22 ss with room for the float64 roundings."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_sim as ws
from oracle import oracle
from svdfeature_amd import BlockArrays, CSRData
from svdfeature_amd.data import PlusBlock, TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

pytestmark = pytest.mark.gpu

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias")
MB = [("amd:step", "minibatch")]


@pytest.fixture(scope="module", autouse=True)
def _port():
    oracle.build()


def _make(cls, conf, fmt=0, active=0, extra=(), knobs=()):
    t = cls(fmt, active) if cls is sa.Trainer else cls("port", fmt, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _port_of(t, conf, fmt=0, active=0):
    """the pinned C port holding the engine's model as its views report it now"""
    o = _make(oracle.OracleTrainer, conf, fmt, active)
    for name in VIEWS:
        a, b = t.view(name), o.view(name)
        if a is None or b is None or b.size == 0:
            continue
        assert a.size == b.size, name
        o.set_view(name, a)
    return o


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(t, ds, want, labels):
    """predict_dataset == want bit for bit, then the evaluator against the file-order predictions"""
    n = len(want)
    got = t.predict_dataset(ds)
    assert got.shape == (n,)
    bad = np.flatnonzero(got.view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32))
    assert bad.size == 0, "%d of %d predictions differ from the port, first at file row %d: %r vs %r" % (bad.size, n, bad[0], got[bad[0]], want[bad[0]])
    ss, cnt = t.eval_dataset(ds)
    assert cnt == n
    diff = (got - np.asarray(labels, np.float32)).astype(np.float64)   # fp32 difference (the evaluator's), float64 from there on
    ref = float(np.sum(diff * diff))
    ref64 = float(np.sum((got.astype(np.float64) - np.asarray(labels, np.float64)) ** 2))
    print("eval: ss %.17g reference %.17g rel %.3g (difference formed in float64: rel %.3g)" % (ss, ref, abs(ss - ref) / max(ref, 1e-300), abs(ss - ref64) / max(ref64, 1e-300)))
    assert abs(ss - ref) <= 1e-9 * ss
    assert abs(ss - ref64) <= 2.0 ** -22 * ss
    return got


def _train(t, ds, passes=2):
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()


# ------------------------------------------------------------------------------------------------- 1. ratings sequence
@pytest.mark.parametrize("k,active", [(10, 0), (64, 0), (128, 0), (10, 2), (64, 2), (128, 2)])
def test_ratings_sequence_both_builders_equal_the_port(k, active):
    nu, ni, n = 300, 60, 3000
    u, i, r = cases.planted_triples(n, nu, ni, seed=k + active)
    if active == 2:
        r = (r > 3).astype(np.float32)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, active_type=active, base_score="0.5" if active else "3")
    d = CSRData.from_triples(u, i, r)
    preds = []
    for dev in (0, 1):   # host builder, device builder (svdf_k_wbuild.hip)
        t = _make(sa.Trainer, conf, 0, active, MB + [("amd:window", 700)], [("device_window", dev)])
        ds = t.dataset_from_triples(u, i, r)
        assert ds.kind == 8 and ds.num_batches == 5   # five windows, the last one partial
        _train(t, ds)
        preds.append(_check(t, ds, _port_of(t, conf, 0, active).predict_batch(d), r))
    assert _same_bits(preds[0], preds[1])


@pytest.mark.parametrize("dev", [0, 1])
def test_ratings_sequence_with_a_hot_window(dev):
    """Zipf-skewed items and window_hot_sub = 4: the popular items have far more than 4 slots in every 700-row window, so the children are hot
    windows (ordered sub-steps, k_window_apply); scoring reads none of that"""
    nu, ni, n, k = 300, 60, 3000, 64
    u, i, r = cases.planted_triples(n, nu, ni, seed=5, zipf=True)
    assert np.bincount(i[:700]).max() > 40
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    t = _make(sa.Trainer, conf, 0, 0, MB + [("amd:window", 700)], [("device_window", dev), ("window_hot_sub", 4)])
    ds = t.dataset_from_triples(u, i, r)
    assert ds.kind == 8 and ds.num_batches == 5
    _train(t, ds)
    _check(t, ds, _port_of(t, conf).predict_batch(CSRData.from_triples(u, i, r)), r)


# ------------------------------------------------------------------------------------------------- 2. pair sequence
@pytest.mark.parametrize("k,dev,psub", [(64, 0, 0), (64, 1, 0), (128, 0, 0), (128, 1, 0), (64, 1, 3), (128, 0, 3)])
def test_pair_sequence_equals_the_port_on_pairs_as_csr(k, dev, psub):
    nu, ni, n = 200, 50, 2000
    pu, pp, pq = cases.planted_pairs(n, nu, ni, seed=k + dev)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k)
    t = _make(sa.Trainer, conf, 0, 3, MB + [("amd:window", 600)], [("device_window", dev), ("window_pair_sub", psub)])
    ds = t.dataset_from_pairs(pu, pp, pq)
    assert ds.kind == 8 and ds.num_batches == 4
    _train(t, ds)
    _check(t, ds, _port_of(t, conf, 0, 3).predict_batch(sa.pairs_as_csr(pu, pp, pq)), np.ones(n, np.float32))


# ------------------------------------------------------------------------------------------------- 3. csr rows
NP_, NS_, NT_, NA_, NG_ = 60, 100, 40, 30, 6   # private users, shared user ids (B = NP_), tracks, item attribute ids, global ids


def _csr_case(variant, tmp_path, seed):
    """(conf keys beyond the widths, extra set_param keys, CSRData)"""
    rng = np.random.default_rng(seed)
    if variant == "a":     # fixed 4 globals + one item, unit values: the estride layout
        rows = [(float(rng.integers(1, 6)), [(int(g), float(rng.uniform(0.1, 1.0))) for g in sorted(rng.choice(NG_, size=4, replace=False))],
                 [(int(rng.integers(0, NP_ + NS_)), 1.0)], [(int(rng.integers(0, NT_ + NA_)), 1.0)]) for _ in range(600)]
        return [], [], CSRData.from_rows(rows)
    if variant == "b":     # 0-3 globals, 1-2 item entries with values != 1, user values != 1: the rptr layout
        return [], [], ws.table_rows(rng, 600, NP_ + NS_, 0, NT_ + NA_, num_global=NG_, max_g=3, max_shared=0, max_items=2, uvals=True, ivals=True)
    if variant == "c":     # amd:shared_user_from: 0-3 shared ids, the private entry first / middle / last
        d = ws.shared_rows(rng, 600, NP_, NS_, NT_ + NA_, num_global=NG_, max_g=2, max_shared=3, uvals=True, hot=(NP_, NP_ + 1), hot_p=0.6)
        return [], [("amd:shared_user_from", NP_)], d
    assert variant == "d"  # feature_user and feature_item tables, children behind item entries with values != 1
    tu = ws.read_table(ws.write_table(str(tmp_path / "fu.txt"), ws.random_table(rng, NP_ + NS_, NP_, NP_ + NS_, 2, hot=(NP_, NP_ + 1), hot_p=0.7)))
    ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), ws.random_table(rng, NT_, NT_, NT_ + NA_, 3, hot=(NT_, NT_ + 1), hot_p=0.7)))
    d = ws.table_rows(rng, 660, NP_, NS_, NT_, num_global=NG_, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = ws.drop_rows_reaching_twice(d, NP_, tu, ti)
    return [("feature_user", str(tmp_path / "fu.txt")), ("feature_item", str(tmp_path / "fi.txt"))], [("amd:shared_user_from", NP_)], d


@pytest.mark.parametrize("variant,k,nub,hot", [("a", 1, 0, 0), ("a", 64, 1, 0), ("a", 256, 0, 0), ("b", 20, 0, 0), ("b", 64, 1, 0), ("b", 256, 1, 0),
                                               ("c", 1, 1, 0), ("c", 20, 0, 0), ("c", 64, 0, 2), ("c", 256, 1, 2),
                                               ("d", 1, 0, 2), ("d", 20, 1, 0), ("d", 64, 0, 0), ("d", 64, 1, 2), ("d", 256, 0, 2)])
def test_csr_rows_every_window_layout_equals_the_port(tmp_path, variant, k, nub, hot):
    """hot = 2: window_shared_sub = window_item_sub = 2, so the windows carry the hot lanes' marks (ent.pad, uent.pad, child slots <= -2) and
    every contribution keeps a slot; scoring must not read any of it"""
    keys, extra, d = _csr_case(variant, tmp_path, seed=k + nub)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NP_ + NS_, num_item=NT_ + NA_, num_global=NG_, num_factor=k, wd_global="0.002",
                           learning_rate="0.01", no_user_bias=nub) + keys
    knobs = [("window_shared_sub", 2), ("window_item_sub", 2)] if hot else []
    t = _make(sa.Trainer, conf, 0, 0, MB + [("amd:window", 170)] + extra, knobs)
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and ds.num_batches == (d.num_row + 169) // 170 and 3 <= ds.num_batches <= 4
    _train(t, ds)
    _check(t, ds, _port_of(t, conf).predict_batch(d), d.row_label)


# ------------------------------------------------------------------------------------------------- 4. user-group blocks
def _svdpp_blocks(seed):
    """about 120 blocks: split users (START / MIDDLE / END), users without feedback (every 7th), one feedback list longer than 64"""
    nu, ni = 200, 90
    blocks = cases.user_blocks(110, nu, ni, ni, seed=seed, max_rows=9, max_fb=6, split_every=4)
    rng = np.random.default_rng(seed)
    fb = np.sort(rng.choice(ni, size=70, replace=False)).astype(np.uint32)
    rows = [(float(rng.integers(1, 6)), [], [(nu - 1, 1.0)], [(int(rng.integers(0, ni)), 1.0)]) for _ in range(5)]
    at = next(j for j in range(40, len(blocks)) if blocks[j - 1].extend_tag in (TAG_DEFAULT, TAG_END))   # not inside a START .. END span
    blocks.insert(at, PlusBlock(fb, np.full(70, 1.0 / np.sqrt(70.0), np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    return nu, ni, [b for b in blocks if not (b.data.num_row and int(b.data.feat_index[b.data.row_ptr[1]]) == nu - 1 and b.num_ufeedback != 70)]


def _port_blocks(o, blocks):
    return np.concatenate([o.predict_block(b) for b in blocks])


@pytest.mark.parametrize("k,nub,defer", [(16, 0, 1), (16, 1, 0), (64, 0, 0), (64, 1, 1), (192, 0, 1), (192, 1, 0)])
def test_user_group_blocks_equal_the_port_predict_block(k, nub, defer):
    nu, ni, blocks = _svdpp_blocks(seed=k + nub)
    assert {b.extend_tag for b in blocks} == {TAG_DEFAULT, TAG_START, TAG_MIDDLE, TAG_END}
    assert any(b.num_ufeedback == 0 for b in blocks) and any(b.num_ufeedback > 64 for b in blocks) and 100 < len(blocks) < 200
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_ufeedback=ni, no_user_bias=nub,
                           wd_ufeedback="0.004", ufeedback_init_sigma="0.01")
    ba = BlockArrays.from_blocks(blocks)
    t = _make(sa.Trainer, conf, 1, 0, MB + [("amd:window", 150)], [("wunit_defer_fb", defer)])
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches >= 3
    _train(t, ds)
    _check(t, ds, _port_blocks(_port_of(t, conf, 1, 0), blocks), ba.row_label)


# ------------------------------------------------------------------------------------------------- 5. amd:step = auto
def test_auto_step_window_sequence_of_rank_pairs_scores():
    """tests/test_gpu_auto_step.py: user-grouped pairs are one dependency chain per user, the estimator takes the window step"""
    from test_gpu_auto_step import _grouped_pairs
    nu, ni = 120, 400
    pu, pp, pq = _grouped_pairs(nu, ni, 500, 7)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=128)
    t = _make(sa.Trainer, conf, 0, 3, [("amd:step", "auto")])
    ds = t.dataset_from_pairs(pu, pp, pq)
    assert ds.kind == 8 and t.counter(16) == 2
    _train(t, ds, 1)
    _check(t, ds, _port_of(t, conf, 0, 3).predict_batch(sa.pairs_as_csr(pu, pp, pq)), np.ones(len(pu), np.float32))


def test_auto_step_window_sequence_of_rows_with_globals_scores():
    from test_gpu_wunit import _rows_with_globals
    d = _rows_with_globals(20000, 300, 200, 8, 3, seed=1, fixed=True)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=300, num_item=200, num_global=8, num_factor=32, wd_global=0.001)
    t = _make(sa.Trainer, conf, 0, 0, [("amd:step", "auto")])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and t.counter(16) == 2
    _train(t, ds, 1)
    _check(t, ds, _port_of(t, conf).predict_batch(d), d.row_label)


# ------------------------------------------------------------------------------------------------- 6. stand-alone windows of a plain handle
@pytest.mark.parametrize("dev", [0, 1])
def test_stand_alone_rating_window_also_between_train_and_apply(dev):
    nu, ni, n, k = 150, 40, 900, 64
    u, i, r = cases.planted_triples(n, nu, ni, seed=3)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    d = CSRData.from_triples(u, i, r)
    t = _make(sa.Trainer, conf, knobs=[("device_window", dev)])
    warm = t.dataset_from_triples(u, i, r)   # an exact pass first: the model is not the initial one
    t.train_dataset(warm)
    ds = t.dataset_window_from_triples(u, i, r)
    assert ds.kind == 5
    users_before = t.view("W_user").copy()
    items_before = t.view("W_item").copy()
    before = _check(t, ds, _port_of(t, conf).predict_batch(d), r)
    # the first half of the window step: the users have moved, the item-side sums are not applied -- the window is scored against the
    # model as the views report it at this moment
    t.train_dataset(ds)
    assert not _same_bits(users_before, t.view("W_user")) and _same_bits(items_before, t.view("W_item"))
    after = _check(t, ds, _port_of(t, conf).predict_batch(d), r)
    assert not _same_bits(before, after)


@pytest.mark.parametrize("dev", [0, 1])
def test_stand_alone_pair_window(dev):
    nu, ni, n, k = 120, 50, 800, 128
    pu, pp, pq = cases.planted_pairs(n, nu, ni, seed=4)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k)
    t = _make(sa.Trainer, conf, 0, 3, knobs=[("device_window", dev)])
    t.train_dataset(t.dataset_from_pairs(pu, pp, pq))
    ds = t.dataset_window_from_pairs(pu, pp, pq)
    assert ds.kind == 5
    _check(t, ds, _port_of(t, conf, 0, 3).predict_batch(sa.pairs_as_csr(pu, pp, pq)), np.ones(n, np.float32))


def test_stand_alone_csr_window():
    _, _, d = _csr_case("b", None, seed=9)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NP_ + NS_, num_item=NT_ + NA_, num_global=NG_, num_factor=20, wd_global="0.002")
    t = _make(sa.Trainer, conf)
    t.train_dataset(t.dataset_from_csr(d))
    ds = t.dataset_window_from_csr(d)
    assert ds.kind == 7
    _check(t, ds, _port_of(t, conf).predict_batch(d), d.row_label)


def test_stand_alone_block_window():
    nu, ni, blocks = _svdpp_blocks(seed=2)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64, num_ufeedback=ni, wd_ufeedback="0.004", ufeedback_init_sigma="0.01")
    ba = BlockArrays.from_blocks(blocks)
    t = _make(sa.Trainer, conf, 1, 0)
    t.train_dataset(t.dataset_from_blocks(ba))
    ds = t.dataset_window_from_blocks(ba)
    assert ds.kind == 7
    _check(t, ds, _port_blocks(_port_of(t, conf, 1, 0), blocks), ba.row_label)


# ------------------------------------------------------------------------------------------------- 7. edges
def test_one_row_data_sets():
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=8, num_item=5, num_factor=10)
    u, i, r = np.array([3], np.uint32), np.array([2], np.uint32), np.array([4.0], np.float32)
    t = _make(sa.Trainer, conf, 0, 0, MB)
    ds = t.dataset_from_triples(u, i, r)
    assert ds.kind == 8 and ds.num_row == 1
    _train(t, ds)
    _check(t, ds, _port_of(t, conf).predict_batch(CSRData.from_triples(u, i, r)), r)
    gconf = cases.conf_with(conf, num_global=3)
    d = CSRData.from_rows([(2.0, [(1, 0.5)], [(7, 0.5)], [(0, 1.0), (4, -0.5)])])
    t = _make(sa.Trainer, gconf, 0, 0, MB)
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and ds.num_row == 1
    _train(t, ds)
    _check(t, ds, _port_of(t, gconf).predict_batch(d), d.row_label)


def test_sequence_of_one_row_windows():
    nu, ni, n = 20, 9, 37
    u, i, r = cases.planted_triples(n, nu, ni, seed=8)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64)
    t = _make(sa.Trainer, conf, 0, 0, MB + [("amd:window", 1)])
    ds = t.dataset_from_triples(u, i, r)
    assert ds.kind == 8 and ds.num_batches == n
    _train(t, ds)
    _check(t, ds, _port_of(t, conf).predict_batch(CSRData.from_triples(u, i, r)), r)


def test_closed_and_rebuilt_and_scoring_leaves_training_alone():
    """train, score, train again == train twice without scoring, bit for bit in every parameter array; a data set closed and built again scores
    the same"""
    _, extra, d = _csr_case("c", None, seed=11)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NP_ + NS_, num_item=NT_ + NA_, num_global=NG_, num_factor=64, wd_global="0.002")
    models = []
    for score in (False, True):
        t = _make(sa.Trainer, conf, 0, 0, MB + [("amd:window", 170)] + extra)
        ds = t.dataset_from_csr(d)
        t.train_dataset(ds)
        if score:
            p1 = t.predict_dataset(ds)
            t.eval_dataset(ds)
            ds.close()
            ds = t.dataset_from_csr(d)
            assert _same_bits(p1, t.predict_dataset(ds))
        t.train_dataset(ds)
        t.synchronize()
        models.append({name: t.view(name).copy() for name in ("W_user", "u_bias", "W_item", "i_bias", "g_bias")})
    for name in models[0]:
        assert _same_bits(models[0][name], models[1][name]), name
    _check(t, ds, _port_of(t, conf).predict_batch(d), d.row_label)

"""Ordered sub-steps for the hot items of a one-GPU window sequence (svdf_k_window.hip: k_window_apply; svdf_wseq_rule.h: wseq_rule_columns; round 6,
VERDICT round 5 item 4).  `amd:step = minibatch / auto` on plain ratings: a window is cut by what the cold rows tolerate; an item with more than
`window_hot_sub` slots in a window is applied by one workgroup in file order, window_hot_sub slots at a time, every sub-step's changes computed against
the row as the previous sub-step left it.  The checker is oracle/svdf_oracle.c: svdo_update_window_substeps (the reference's update_inner, apex_svd_base.h:
456-462, per row -- users against the window-start item side, the item side per sub-step): the model must equal it bit for bit."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_item", "i_bias", "W_user", "u_bias")


def _trainer(conf, active=0, extra=(), knobs=()):
    t = sa.Trainer(0, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _oracle(conf, active, u, i, r, windows, sub, passes):
    from oracle import oracle
    oracle.build()
    o = oracle.OracleTrainer("port", 0, active)
    o.seed(10)
    for k, v in conf:
        o.set_param(k, v)
    o.init_model()
    o.init_trainer()
    n = len(r)
    ws = [sa.CSRData.from_triples(u[n * w // windows:n * (w + 1) // windows], i[n * w // windows:n * (w + 1) // windows], r[n * w // windows:n * (w + 1) // windows])
          for w in range(windows)]
    for _ in range(passes):
        for d in ws:
            o.update_window_substeps(d, sub)
    return o


@pytest.mark.parametrize("k,active,extra,sub", [(64, 0, (), 16), (128, 0, (), 16), (64, 0, (), 128), (24, 0, (), 16), (40, 0, (("no_user_bias", "1"),), 8),
                                              (32, 2, (("base_score", "0.5"),), 16), (256, 0, (), 24), (8, 0, (("reg_method", "1"),), 16), (64, 0, (("wd_item", "0.02"), ("wd_user", "0.01")), 40),
                                              (128, 0, (), 200), (256, 0, (), 100)])   # (a sub-step of several rounds of the workgroup: three full ones and one of 8 / of 4)
def test_hot_items_move_in_ordered_sub_steps_and_equal_the_checker(k, active, extra, sub):
    nu, ni, n, passes = 3000, 150, 60000, 2
    u, i, r = cases.planted_triples(n, nu, ni, seed=k + sub, zipf=True)
    if active == 2:
        r = (r > 3).astype(np.float32)
    cnt = np.bincount(i, minlength=ni)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k) + [(a, b) for a, b in extra]
    t = _trainer(conf, active, [("amd:step", "minibatch")], [("window_hot_sub", sub), ("window_hot_max", 20 * sub), ("window_per_target", 100000)])   # (the mean rule out of the way: the windows come from window_hot_max)
    ds = t.dataset_from_triples(u, i, r)
    W = ds.num_batches
    assert ds.kind == 8 and cnt.max() / W > 2 * sub, (cnt.max(), W)       # the top item takes several sub-steps per window
    assert W <= -(-cnt.max() // (20 * sub)) * 4                           # ... and the windows are cut by the hot-lane rule, not by 128 per row
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    o = _oracle(conf, active, u, i, r, W, sub, passes)
    for name in NAMES:
        a, b = t.view(name), o.view(name)
        assert np.isfinite(a).all(), name
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, W)


def test_windows_without_a_hot_item_and_the_switch():
    """uniform ratings: no window holds a hot item, the sequence is the round-5 one (same windows, same bits: the one-rank stale simulation);
    window_hot_sub = 0 switches the lane off and restores the round-5 rule (no row more than window_per_target_max per window)"""
    nu, ni, n = 2000, 400, 40000
    u, i, r = cases.planted_triples(n, nu, ni, seed=3)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64)
    models = []
    for sub in (128, 0):
        t = _trainer(conf, 0, [("amd:step", "minibatch")], [("window_hot_sub", sub)])
        ds = t.dataset_from_triples(u, i, r)
        t.train_dataset(ds)
        t.synchronize()
        models.append((ds.num_batches, {nm: t.view(nm).copy() for nm in NAMES}))
    assert models[0][0] == models[1][0]
    for nm in NAMES:
        assert np.array_equal(models[0][1][nm].view(np.uint32), models[1][1][nm].view(np.uint32)), nm
    # skewed: far fewer windows with the lane than without
    u, i, r = cases.planted_triples(400000, 20000, 20000, seed=5, zipf=True)   # (top item ~3 % of the ratings among 20 000 items)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=20000, num_item=20000, num_factor=64)
    nw = []
    for sub in (128, 0):
        t = _trainer(conf, 0, [("amd:step", "minibatch")], [("window_hot_sub", sub)])
        nw.append(t.dataset_from_triples(u, i, r).num_batches)
    assert nw[0] * 2 < nw[1], nw


def test_the_hot_lane_keeps_the_accuracy_contract_on_skewed_items():
    """Zipf items, 2 M ratings: held-out RMSE of the sub-step sequence within 1e-4 of the exact sequential pass after 3 passes (the contract of every
    window step), finite everywhere -- the condition the round-5 cap existed for (stale sums of a hot row diverge)"""
    nu, ni, n = 100000, 5000, 2000000
    u, i, r = cases.planted_triples(n + 100000, nu, ni, seed=21, zipf=True)
    test = sa.CSRData.from_triples(u[n:], i[n:], r[n:])
    tl = r[n:]
    u, i, r = u[:n], i[:n], r[:n]
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64)
    out = []
    for extra in ([], [("amd:step", "minibatch")]):
        t = _trainer(conf, 0, extra)
        ds = t.dataset_from_triples(u, i, r)
        for _ in range(3):
            t.train_dataset(ds)
        p = t.predict_batch(test)
        assert np.isfinite(p).all()
        out.append((float(np.sqrt(np.mean((p.astype(np.float64) - tl) ** 2))), ds.num_batches, ds.kind))
    assert out[1][2] == 8
    assert abs(out[1][0] - out[0][0]) <= 1e-4, out


def test_random_shapes_against_the_checker():
    """twenty random (users, items, ratings, width, sub-step, cap, passes) draws over Zipf items -- incl. windows without any hot item, sub-steps that do not
    divide the slot counts, widths that are not a multiple of 4, caps below the sub-step (every item of a window hot) -- each equal to the checker bit for bit"""
    rng = np.random.default_rng(2026)
    for case in range(20):
        nu, ni = int(rng.integers(50, 3000)), int(rng.integers(5, 400))
        n = int(rng.integers(2000, 40000))
        k = int(rng.choice([3, 8, 16, 24, 32, 64, 64, 100, 128, 200]))
        sub = int(rng.choice([1, 3, 8, 16, 33, 64, 128]))
        cap = int(sub * rng.choice([0.5, 1, 2, 7, 20]) + 1)
        passes = int(rng.integers(1, 3))
        u, i, r = cases.planted_triples(n, nu, ni, seed=1000 + case, zipf=bool(rng.integers(0, 4)))
        extra = [("no_user_bias", "1")] if rng.integers(0, 5) == 0 else []
        conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, learning_rate=0.002) + extra
        # (window_count_actual 0: the draws pick caps down to ONE update per window so that every item of a window is hot; held on the windows as
        # cut, such a cap means one rating per window -- up to 38 000 windows here and no hot item left to check.  tests/test_gpu_window_orders.py
        # runs the lane under the rule as it is enforced)
        t = _trainer(conf, 0, [("amd:step", "minibatch")], [("window_hot_sub", sub), ("window_hot_max", cap), ("window_per_target", 100000), ("window_count_actual", 0)])
        ds = t.dataset_from_triples(u, i, r)
        W = ds.num_batches
        for _ in range(passes):
            t.train_dataset(ds)
        t.synchronize()
        o = _oracle(conf, 0, u, i, r, W, sub, passes)
        for name in NAMES:
            a, b = t.view(name), o.view(name)
            if a is None and b is None:
                continue
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (case, name, nu, ni, n, k, sub, cap, W)
        t.close()

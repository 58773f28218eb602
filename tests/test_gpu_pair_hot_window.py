"""Ordered sub-steps for hot items of rank pairs in the one-GPU window step (`amd:step = minibatch`, knobs `window_pair_sub` /
`window_pair_max`; svdf_wseq.cpp: wseq_from_pairs, svdf_k_window.hip: k_window_apply_pairs / k_window_pair_sums).  An
item with more than window_pair_sub slots in a window -- both signs counted -- is applied in file order, that many slots at a time, every
sub-step's changes formed against the row as the previous sub-step left it and against the OTHER item's window-start row; everything else
moves as in the plain window step.  Every view must equal the checker of tests/window_sim.py on the pair-shaped rows (tests/pair_hot_cases.py)
bit for bit.  With the knob at 0 (the default) nothing changes."""
import numpy as np
import pytest

import cases
import pair_hot_cases as ph
import svdfeature_amd as sa
import window_rule as wr

pytestmark = pytest.mark.gpu

NU, NI = ph.NU, ph.NI
MB = [("amd:step", "minibatch")]


def _trainer(conf, extra=(), knobs=(), fmt=0):
    active = int(dict(conf).get("active_type", 0))
    t = sa.Trainer(fmt, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _bits(t):
    t.synchronize()
    return {name: t.view(name).copy() for name in ph.VIEWS}


def _same_bits(a, b):
    for name in ph.VIEWS:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def _assert_same(t, o):
    t.synchronize()
    for name in ph.VIEWS:
        assert np.array_equal(t.view(name).view(np.uint32), o.view(name).view(np.uint32)), name


def _run(k, active, reg, extra, s, window=90, n=330, passes=2, seed=None, **draw):
    """one case: the pairs, two passes on the GPU against the checker and against the plain window step; returns what the pairs hold"""
    extra = ph.ip_ranges() if extra == "ip" else extra
    rng = np.random.default_rng(2000 + k + reg + s if seed is None else seed)
    u, p, q = ph.draw_pairs(rng, n, **draw)
    conf = ph.conf(k, active, reg, extra)
    t = _trainer(conf, MB + [("amd:window", window)], [("window_pair_sub", s)])
    ds = t.dataset_from_pairs(u, p, q)
    W = ds.num_batches
    assert ds.kind == 8 and W == (n + window - 1) // window   # with amd:window the window size is the caller's
    for _ in range(passes):
        t.train_dataset(ds)
    o = ph.check(conf, u, p, q, W, passes, s)
    _assert_same(t, o)
    # the lane did something: the plain window step ends elsewhere
    plain = ph.check(conf, u, p, q, W, passes, 0)
    assert not np.array_equal(plain.view("W_item")[:3], o.view("W_item")[:3])
    return ph.facts(p, q, W, s)


NUB = (("no_user_bias", "1"),)
# (k, active_type, reg_method, extra keys, window_pair_sub)
PARITY = [
    (1, 3, 0, (), 1),
    (3, 0, 1, (("wd_item_bias", "0.01"),), 3),
    (7, 2, 3, NUB, 5),
    (16, 3, 2, "ip", 12),
    (64, 3, 0, NUB, 5),                                   # the slots walk (k = 64, sigmoid rank loss, no user bias)
    (64, 3, 0, "ip", 12),
    (64, 0, 1, NUB + (("wd_item_bias", "0.02"),), 3),
    (100, 2, 3, "ip", 1),
    (128, 3, 0, NUB, 5),                                  # the contract shape: the slots walk at k = 128
    (128, 3, 0, NUB + (("wd_item_bias", "0.01"),), 12),
    (128, 3, 2, (), 3),
    (200, 0, 2, (("user_nonnegative", "1"),), 12),
    (256, 3, 1, "ip", 5),
    (256, 2, 0, (("wd_user_bias", "0.005"), ("wd_item_bias", "0.01")), 1),
]


@pytest.mark.parametrize("k,active,reg,extra,s", PARITY)
def test_hot_items_of_pairs_in_sub_steps_equal_the_checker(k, active, reg, extra, s):
    f = _run(k, active, reg, extra, s)
    assert f["nhot"] >= 8 and (f["ragged"] or s == 1)
    assert f["two_hot"] > 0
    assert f["as_lo"] and f["as_hi"] and f["as_pos"] and f["as_neg"]


@pytest.mark.parametrize("k", [16, 128, 256])
def test_one_window_with_sub_steps_of_128_spans_lane_group_rounds(k):
    """window_pair_sub = 128 on a single 330-pair window: one item is the positive one with p = 0.9, so its list holds two full sub-steps (several
    rounds of the workgroup's lane groups each at k = 128 / 256) and ends on a partial round"""
    f = _run(k, 3, 0, NUB, 128, window=330, seed=77, p_pos=0.9, p_neg=0.0, hot=(1,))
    assert f["nhot"] == 1 and f["most"] > 128 + 16 and (f["most"] % 128) % 16 != 0


def _uniform(n, ni, seed):
    rng = np.random.default_rng(seed)
    return ph.draw_pairs(rng, n, hot=(), ni=ni)


def test_knob_at_zero_is_the_knob_unset_and_cold_windows_keep_their_bits():
    u, p, q = ph.draw_pairs(np.random.default_rng(5), 2000)
    conf = ph.conf(32)
    got = []
    for knobs in ((), (("window_pair_sub", 0),), (("window_pair_sub", 0), ("window_pair_max", 32))):
        t = _trainer(conf, MB, knobs)
        ds = t.dataset_from_pairs(u, p, q)
        for _ in range(2):
            t.train_dataset(ds)
        got.append((ds.kind, ds.num_batches, _bits(t)))
    assert got[0][:2] == got[1][:2] == got[2][:2] and got[0][0] == 8 and got[0][1] > 1
    _same_bits(got[0][2], got[1][2])
    _same_bits(got[0][2], got[2][2])
    # knob on, but no window holds a hot item: the plain launches, the same bits as knob off under the same amd:window
    ni = 400
    u, p, q = _uniform(2000, ni, 6)
    assert ph.facts(p, q, 10, 12)["nhot"] == 0
    conf = ph.conf(64, 3, 0, NUB, ni=ni)
    res = []
    for s in (0, 12):
        t = _trainer(conf, MB + [("amd:window", 200)], [("window_pair_sub", s)])
        ds = t.dataset_from_pairs(u, p, q)
        assert ds.num_batches == 10
        for _ in range(2):
            t.train_dataset(ds)
        res.append(_bits(t))
    _same_bits(res[0], res[1])


def test_window_rule_with_sub_steps():
    u, p, q = ph.draw_pairs(np.random.default_rng(8), 4000)
    counts = np.bincount(np.concatenate([p, q]).astype(np.int64), minlength=NI)
    t = _trainer(ph.conf(16), MB)
    default = t.dataset_from_pairs(u, p, q).num_batches
    assert default == wr.columns(len(u), counts) and default > 8
    seen = set()
    for s, cap in ((5, 2048), (5, 64), (30, 2048), (128, 512), (12, 100), (24, 200)):
        t.set_knob("window_pair_sub", s)
        t.set_knob("window_pair_max", cap)
        W = t.dataset_from_pairs(u, p, q).num_batches
        assert W == wr.columns(len(u), counts, (s, cap)), (s, cap)
        seen.add(W)
    assert len(seen) >= 4 and 1 in seen
    # amd:window overrides the count, and rows over the threshold still ride the lane (the parity cases above run under amd:window)
    t = _trainer(ph.conf(16), MB + [("amd:window", 300)], [("window_pair_sub", 5), ("window_pair_max", 64)])
    assert t.dataset_from_pairs(u, p, q).num_batches == 14


def test_train_dataset_refuses_a_knob_changed_since_the_build():
    u, p, q = ph.draw_pairs(np.random.default_rng(9), 600)
    t = _trainer(ph.conf(8), MB, [("window_pair_sub", 8)])
    ds = t.dataset_from_pairs(u, p, q)
    t.train_dataset(ds)
    for other in (3, 0):
        t.set_knob("window_pair_sub", other)
        with pytest.raises(sa.SvdfError, match="built with another window_pair_sub"):
            t.train_dataset(ds)
    t.set_knob("window_pair_sub", 8)
    t.train_dataset(ds)
    t.synchronize()
    # a sequence built with the knob off is refused once it is on
    t.set_knob("window_pair_sub", 0)
    ds0 = t.dataset_from_pairs(u, p, q)
    t.set_knob("window_pair_sub", 8)
    with pytest.raises(sa.SvdfError, match="built with another window_pair_sub"):
        t.train_dataset(ds0)
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub must be in 0 \.\. 128"):
        t.set_knob("window_pair_sub", 129)
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub must be in 0 \.\. 128"):
        t.set_knob("window_pair_sub", -1)
    with pytest.raises(sa.SvdfError, match="window_pair_max must be positive"):
        t.set_knob("window_pair_max", 0)


def test_refusals_name_their_cause():
    u, p, q = ph.draw_pairs(np.random.default_rng(10), 50)
    # bf16 contribution rows
    t = _trainer(ph.conf(8), MB + [("amd:contrib", "bf16")], [("window_pair_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub > 0 \(ordered sub-steps for hot items of rank pairs\) needs amd:contrib = fp32"):
        t.dataset_from_pairs(u, p, q)
    # the N-rank wire layout
    t = _trainer(ph.conf(8), [], [("window_pair_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"svdf_dataset_window_from_pairs: window_pair_sub > 0 .* is for the one-GPU window sequence"):
        t.dataset_window_from_pairs(u, p, q)
    t.set_knob("window_pair_sub", 0)
    t.dataset_window_from_pairs(u, p, q).close()
    # amd:gpus > 1 (virtual ranks on a one-GPU machine)
    m = _trainer(ph.conf(8), [("amd:gpus", 2)])
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub > 0 .* amd:gpus > 1"):
        m.set_knob("window_pair_sub", 12)
    # user-group (SVD++) trainers
    g = _trainer(cases.conf_with(ph.conf(8), num_ufeedback=NI), MB, [("window_pair_sub", 12)], fmt=1)
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub > 0 .* is not supported with user-group \(SVD\+\+\) trainers"):
        g.dataset_from_pairs(u, p, q)


def test_the_staged_route_honours_the_knob():
    """update_csr_batch under amd:step = minibatch with the knob == the resident route built chunk by chunk from the same cuts (the pattern of
    tests/test_gpu_staged_window.py), and != the same feed with the knob at 0"""
    from test_gpu_staged_window import _cuts, _feed, _resident, _same, _views, _differ
    S, batch, s = 1024, 500, 8
    u, p, q = ph.draw_pairs(np.random.default_rng(11), 2600)
    d = sa.pairs_as_csr(u, p, q)
    conf = ph.conf(32, 3, 0, NUB)
    make = lambda sub: _trainer(conf, MB + [("amd:window", 256)], [("stage_window", S), ("window_pair_sub", sub)])   # noqa: E731
    cuts = _cuts(d.num_row, batch, S)
    assert len(cuts) >= 2
    assert ph.facts(p[:256], q[:256], 1, s)["nhot"] >= 1
    t = make(s)
    _feed(t, d, batch)
    r = _resident(make(s), d, cuts, lambda t_, a, b: t_.dataset_from_pairs(u[a:b], p[a:b], q[a:b]))
    z = make(0)
    _feed(z, d, batch)
    got = _views(t, ph.VIEWS)
    assert all(np.isfinite(v).all() for v in got.values())
    _same(got, _views(r, ph.VIEWS))
    assert _differ(got, _views(z, ph.VIEWS))
    assert t.counter(30) == len(cuts) and t.counter(31) == 0


def test_staged_chunks_with_bf16_slots_keep_the_exact_step(capfd):
    """window_pair_sub > 0 with amd:contrib = bf16: decided before the build -- the chunks train exactly, nothing raises"""
    from test_gpu_staged_window import _cuts, _feed, _same, _views
    u, p, q = ph.draw_pairs(np.random.default_rng(12), 1500)
    d = sa.pairs_as_csr(u, p, q)
    conf = ph.conf(16, 3, 0, NUB)
    knobs = [("stage_window", 1024), ("window_pair_sub", 8)]
    t = _trainer(conf, MB + [("amd:contrib", "bf16")], knobs)
    e = _trainer(conf, [("amd:contrib", "bf16")], knobs)
    _feed(t, d, 500)
    _feed(e, d, 500)
    _same(_views(t, ph.VIEWS), _views(e, ph.VIEWS))
    assert t.counter(30) == 0 and t.counter(31) == len(_cuts(d.num_row, 500, 1024))
    assert "window_pair_sub" in capfd.readouterr().err


def test_short_fuzz_run():
    import fuzz_pair_hot
    assert fuzz_pair_hot.run(iters=20, seed=7) == 0

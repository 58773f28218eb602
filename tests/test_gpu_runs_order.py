"""Order of the runs inside a level (knob runs_order; svdf_runs.cpp, svdf_k_runs.hip: k_runs_order_key / k_runs_order_stats): a
wave of k_basicmf_runs_soa carries 8 runs (4 at k = 128) and walks as many steps as the longest, so a level's runs are sorted longest first, by item inside
a length, and the sorted row sets are dealt into the eight contiguous shares the XCDs take (k_runs_order_deal).  The units of a level commute: the model must equal, bit for bit, the item-ordered pass (runs_order = 0), the pass on rows in W and the
level-by-level pass over single instances (runs_exec = 0) after three passes with W changed in between, and the oracle after one.  The two dataset facts
runs_wave_steps (11) / runs_mixed_sets (12) are what the order is for: checked against their bounds, and against exact values where every run has one length."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_user", "W_item", "u_bias", "i_bias")
WAVE_STEPS, MIXED_SETS, ORDER = 11, 12, 13
VARIANTS = {
    "order 1, staged": [("runs_exec", 1), ("runs_order", 1), ("runs_stage", 1)],
    "order 1, rows in W": [("runs_exec", 1), ("runs_order", 1), ("runs_stage", 0)],
    "order 0": [("runs_exec", 1), ("runs_order", 0), ("runs_stage", 1)],
    "levels of single instances": [("runs_exec", 0)],
}
# never symmetric: different row decays, nonzero different bias decays, another learning rate and base score (tests/forms_cases.py)
ASYMMETRIC = dict(wd_user=0.02, wd_item=0.003, wd_user_bias=0.01, wd_item_bias=0.004, learning_rate=0.01, base_score=1.7)


def _setup(t, nu, ni, k, conf):
    t.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, **conf):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    return t


def _run(u, i, r, nu, ni, knobs, k, conf, other):
    """three passes; between the first two W changes behind the data set's back (a pass over `other`, one update()).  -> (model after pass 1, after pass 3, ds)"""
    t = _setup(sa.Trainer(0, 0), nu, ni, k, conf)
    for kk, v in [("pivot_exec", 0), ("runs_min_rows", 0)] + knobs:
        t.set_knob(kk, v)
    ds = t.dataset_from_triples(u, i, r)
    ds2 = t.dataset_from_triples(*other)
    first = None
    for p in range(3):
        t.train_dataset(ds)
        if p == 0:
            t.synchronize()
            first = {n: t.view(n).copy() for n in NAMES}
            t.train_dataset(ds2)
            t.update_batch(sa.CSRData.from_triples(other[0][:7], other[1][:7], other[2][:7]))
    t.synchronize()
    return first, {n: t.view(n).copy() for n in NAMES}, ds


def _same(a, b, what):
    for name in NAMES:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), (what, name)


def _check(u, i, r, nu, ni, knobs=(), k=64, conf=None):
    """the four passes agree, the first equals the oracle; -> {variant: data set} for the order facts"""
    from oracle import oracle
    oracle.build()
    conf = conf or {}
    rng = np.random.default_rng(len(u))
    m = max(len(u) // 10, 8)
    other = (rng.integers(0, nu, m).astype(np.uint32), rng.integers(0, ni, m).astype(np.uint32), rng.integers(1, 6, m).astype(np.float32))
    got = {name: _run(u, i, r, nu, ni, kn + (list(knobs) if kn[0][1] else []), k, conf, other) for name, kn in VARIANTS.items()}
    ds = {name: g[2] for name, g in got.items()}
    assert [d.kind for d in ds.values()] == [10, 10, 10, 0]
    assert [d.info(ORDER) for d in ds.values()] == [1, 1, 0, -1]
    ref = got["order 1, staged"]
    assert ref[2].info(9) == 1   # staging built
    for name in list(VARIANTS)[1:]:
        _same(ref[0], got[name][0], name + ", one pass")
        _same(ref[1], got[name][1], name + ", three passes")
    o = _setup(oracle.OracleTrainer("port", 0, 0), nu, ni, k, conf)
    o.update_batch(sa.CSRData.from_triples(u, i, r))
    _same(ref[0], {n: o.view(n) for n in NAMES}, "the oracle, one pass")
    # the order's facts: what a pass walks under either order
    d1, d0 = ds["order 1, staged"], ds["order 0"]
    rf = dict(knobs).get("runs_len", 4)
    width = 2 if rf <= 2 else (4 if rf <= 4 else 7)
    assert d1.num_batches == d0.num_batches and d1.info(5) == d0.info(5)
    assert d1.info(WAVE_STEPS) == ds["order 1, rows in W"].info(WAVE_STEPS)
    assert 0 <= d1.info(MIXED_SETS) <= (width - 1) * d1.num_batches
    assert 0 < d1.info(WAVE_STEPS) <= d0.info(WAVE_STEPS)
    return ds


def _random(n, nu, ni, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, nu, n).astype(np.uint32), rng.integers(0, ni, n).astype(np.uint32), rng.integers(1, 6, n).astype(np.float32)


def test_levels_smaller_than_one_row_set():
    u, i, r = _random(40, 10, 8, 1)
    _check(u, i, r, 10, 8)


@pytest.mark.parametrize("k", [64, 128])
def test_class_cuts_in_the_middle_of_row_sets(k):
    """levels of up to 40 runs (one per item) of every length: the lengths' boundaries fall inside row sets of 8 (k = 64) and of 4 (k = 128)"""
    u, i, r = _random(60000, 3000, 40, 2)
    ds = _check(u, i, r, 3000, 40, k=k)
    assert ds["order 1, staged"].info(WAVE_STEPS) < ds["order 0"].info(WAVE_STEPS)   # mixed lengths: the order saves steps here


@pytest.mark.parametrize("k", [64, 128])
def test_levels_of_many_row_sets(k):
    """levels of up to 1000 runs, 125 (250) row sets: every XCD's share of the dealt order holds several sets of every length; 1003 is no multiple of 8 or 4"""
    u, i, r = _random(120000, 20000, 1003, 7)
    ds = _check(u, i, r, 20000, 1003, k=k)
    assert ds["order 1, staged"].info(WAVE_STEPS) < ds["order 0"].info(WAVE_STEPS)


def _sets(level_sizes, ips):
    return sum((s + ips - 1) // ips for s in level_sizes)


@pytest.mark.parametrize("k,ips", [(64, 8), (128, 4)])
def test_all_runs_of_length_one(k, ips):
    """every item is rated by one user only: a user's second rating of the item cannot join a run that holds its first.  Level l = the l-th rating of
    every item that has one, so runs_wave_steps = the row sets of those levels, one step each"""
    ni = 37
    rng = np.random.default_rng(3)
    count = rng.integers(1, 30, ni)
    i = rng.permutation(np.repeat(np.arange(ni), count)).astype(np.uint32)
    u = i.copy()
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    ds = _check(u, i, r, ni, ni, k=k)
    sizes = [int((count > l).sum()) for l in range(int(count.max()))]
    for d in (ds["order 1, staged"], ds["order 0"]):
        assert d.num_batches == len(sizes) and d.info(5) == len(i)
        assert d.info(WAVE_STEPS) == _sets(sizes, ips) and d.info(MIXED_SETS) == 0


@pytest.mark.parametrize("k,ips,rl", [(64, 8, 4), (128, 4, 4), (64, 8, 7)])
def test_all_runs_of_full_length(k, ips, rl):
    """every user rates once and every item a multiple of runs_len times: each item's ratings are cut into full runs, level l = the l-th run of every item"""
    ni, m = 29, 5
    rng = np.random.default_rng(4)
    i = rng.permutation(np.repeat(np.arange(ni), rl * m)).astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    ds = _check(u, i, r, len(i), ni, knobs=[("runs_len", rl)], k=k)
    for d in (ds["order 1, staged"], ds["order 0"]):
        assert d.num_batches == m and d.info(5) == ni * m
        assert d.info(WAVE_STEPS) == _sets([ni] * m, ips) * rl and d.info(MIXED_SETS) == 0


@pytest.mark.parametrize("rl", [2, 3, 4, 6, 7])
def test_every_width(rl):
    u, i, r = cases.planted_triples(30000, 2000, 60, seed=10 + rl, zipf=True)
    _check(u, i, r, 2000, 60, knobs=[("runs_len", rl)])


@pytest.mark.parametrize("knobs", [
    [("runs_sets", 2)],
    [("runs_block", 128)],
    [("runs_block", 256), ("xcd_remap", 1)],          # the grid is padded past the level's end
    [("runs_sets", 2), ("runs_block", 256), ("xcd_remap", 1), ("runs_len", 7)],
])
def test_launch_shapes(knobs):
    u, i, r = _random(50000, 2500, 50, 5)
    _check(u, i, r, 2500, 50, knobs=knobs)


@pytest.mark.parametrize("k", [64, 128])
def test_asymmetric_parameters(k):
    u, i, r = cases.planted_triples(40000, 3000, 150, seed=6, zipf=True)
    r = (r + np.random.default_rng(6).uniform(-0.5, 0.5, len(r)) - 2.25).astype(np.float32)   # real-valued labels, some negative
    _check(u, i, r, 3000, 150, k=k, conf=ASYMMETRIC)

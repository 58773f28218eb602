"""Operand staging of the runs pass (knob runs_stage; svdf_runs.cpp: runs_stage_build, svdf_k_runs.hip: k_runs_stage_in and the STAGED form of
k_basicmf_runs_soa): a run reads its rows and biases from its own schedule slots and writes each into the slot of the row's next
reader, home to W at the row's last touch of the pass.  Same instances, same arithmetic, every row's touches in file order: the model must equal the
runs_stage = 0 pass and the level-by-level pass over single instances (runs_exec = 0) bit for bit -- after three passes (slots are rewritten), with W
changed between passes by another data set and by update() (the stage-in kernel re-reads W), on rows touched once, on rows never touched."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_user", "W_item", "u_bias", "i_bias")
STAGED, IN_W, LEVELS = [("runs_exec", 1), ("runs_stage", 1)], [("runs_exec", 1), ("runs_stage", 0)], [("runs_exec", 0)]
STAGE_STATE, STAGE_BYTES = 9, 10   # Dataset.info: 0 not tried / 1 built / 2 refused; bytes of the staging buffers


def _trainer(nu, ni, knobs, k=64):
    t = sa.Trainer(0, 0)
    t.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    t.set_knob("pivot_exec", 0)
    t.set_knob("runs_min_rows", 0)
    for kk, v in knobs:
        t.set_knob(kk, v)
    return t


def _run(u, i, r, nu, ni, knobs, k=64, passes=3, other=None):
    """`passes` passes over (u, i, r); between the first two, W changes behind the data set's back: a pass over the data set `other` and one update()"""
    t = _trainer(nu, ni, knobs, k)
    ds = t.dataset_from_triples(u, i, r)
    ds2 = t.dataset_from_triples(*other) if other is not None else None
    for p in range(passes):
        t.train_dataset(ds)
        if p == 0 and other is not None:
            t.train_dataset(ds2)
            t.update_batch(sa.CSRData.from_triples(other[0][:7], other[1][:7], other[2][:7]))
    t.synchronize()
    return {n: t.view(n).copy() for n in NAMES}, ds, t


def _same(a, b, what):
    for name in NAMES:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), (what, name)


def _three_ways(u, i, r, nu, ni, knobs, k=64, other=None):
    a, dsa, ta = _run(u, i, r, nu, ni, STAGED + knobs, k, other=other)
    b, dsb, _ = _run(u, i, r, nu, ni, IN_W + knobs, k, other=other)
    c, dsc, _ = _run(u, i, r, nu, ni, LEVELS, k, other=other)
    assert dsa.kind == 10 and dsb.kind == 10 and dsc.kind == 0
    assert dsa.info(STAGE_STATE) == 1 and dsa.info(STAGE_BYTES) > 0 and dsb.info(STAGE_STATE) == 0 and ta.counter(23) == 3 + (other is not None)
    _same(a, b, "staged against rows in W")
    _same(a, c, "staged against the level-by-level pass")
    return a


@pytest.mark.parametrize("nu,ni,n,zipf,knobs", [
    (64, 9, 5000, False, [("runs_len", 6)]),
    (500, 2000, 40000, False, [("runs_len", 3), ("runs_sets", 2), ("runs_block", 128)]),   # many rows touched exactly once: first touch = last touch
    (3000, 40, 60000, True, [("runs_len", 2)]),
    (20000, 300, 300000, True, [("runs_len", 4), ("runs_block", 256)]),
])
def test_staged_passes_equal_the_passes_on_w(nu, ni, n, zipf, knobs):
    u, i, r = cases.planted_triples(n, nu, ni, seed=nu + n, zipf=zipf)
    other = cases.planted_triples(max(n // 10, 8), nu, ni, seed=nu + n + 1, zipf=zipf)
    _three_ways(u, i, r, nu, ni, knobs, other=other)


def test_staged_passes_at_k_128():
    nu, ni, n = 2000, 100, 50000
    u, i, r = cases.planted_triples(n, nu, ni, seed=33)
    other = cases.planted_triples(5000, nu, ni, seed=34)
    _three_ways(u, i, r, nu, ni, [("runs_len", 4)], k=128, other=other)


def test_one_rating():
    u = np.array([3], np.uint32); i = np.array([5], np.uint32); r = np.array([4.0], np.float32)
    _three_ways(u, i, r, 10, 8, [("runs_len", 4)])


def test_a_user_rating_the_same_item_twice_in_a_row_and_other_repeats():
    rng = np.random.default_rng(3)
    nu, ni, n = 50, 12, 6000
    u = rng.integers(0, nu, n).astype(np.uint32)
    i = rng.integers(0, ni, n).astype(np.uint32)
    u[1::7] = u[0::7][:len(u[1::7])]     # the same (user, item) twice in a row, and the same user on consecutive ratings
    i[1::7] = i[0::7][:len(i[1::7])]
    r = rng.integers(1, 6, n).astype(np.float32)
    _three_ways(u, i, r, nu, ni, [("runs_len", 7)])


def test_rows_never_touched_keep_their_bytes():
    nu, ni, n = 300, 50, 8000
    u, i, r = cases.planted_triples(n, 200, 30, seed=5)   # users 200 .., items 30 .. have no rating
    t = _trainer(nu, ni, STAGED + [("runs_len", 4)])
    before = {name: t.view(name).copy() for name in NAMES}
    ds = t.dataset_from_triples(u, i, r)
    for _ in range(3):
        t.train_dataset(ds)
    t.synchronize()
    assert ds.kind == 10 and ds.info(STAGE_STATE) == 1
    for name, cut in (("W_user", 200), ("u_bias", 200), ("W_item", 30), ("i_bias", 30)):
        after = t.view(name)
        assert np.array_equal(after[cut:].view(np.uint32), before[name][cut:].view(np.uint32)), name
        assert not np.array_equal(after[:cut].view(np.uint32), before[name][:cut].view(np.uint32)), name


def test_one_data_set_trained_by_either_kernel():
    """the knob is read at every pass: passes alternate between the staged kernel and the one on W over the SAME data set"""
    nu, ni, n = 3000, 40, 60000
    u, i, r = cases.planted_triples(n, nu, ni, seed=8, zipf=True)
    ref, _, _ = _run(u, i, r, nu, ni, IN_W + [("runs_len", 4)], passes=4)
    for first in (0, 1):   # built with the knob off (staging built at the first staged pass) and with the knob on
        t = _trainer(nu, ni, [("runs_exec", 1), ("runs_stage", first), ("runs_len", 4)])
        ds = t.dataset_from_triples(u, i, r)
        assert ds.info(STAGE_STATE) == first
        for p in range(4):
            t.set_knob("runs_stage", (first + p) % 2)
            t.train_dataset(ds)
        t.synchronize()
        assert ds.info(STAGE_STATE) == 1
        _same({name: t.view(name).copy() for name in NAMES}, ref, "alternating, built with runs_stage = %d" % first)


def test_a_cap_below_the_need_falls_back_to_w():
    nu, ni, n = 20000, 300, 300000
    u, i, r = cases.planted_triples(n, nu, ni, seed=nu + n, zipf=True)
    a, dsa, ta = _run(u, i, r, nu, ni, STAGED + [("runs_len", 4), ("runs_stage_max_mb", 1)], passes=2)
    b, dsb, _ = _run(u, i, r, nu, ni, STAGED + [("runs_len", 4)], passes=2)
    assert dsa.kind == 10 and dsa.info(STAGE_STATE) == 2 and dsa.info(STAGE_BYTES) == 0   # refused: the description says so
    assert dsb.info(STAGE_STATE) == 1 and dsb.info(STAGE_BYTES) > (1 << 20) and ta.counter(23) == 2
    _same(a, b, "fallback against staged")


def test_staged_pass_equals_the_oracle():
    from oracle import oracle
    oracle.build()
    nu, ni, n = 4000, 300, 80000
    u, i, r = cases.planted_triples(n, nu, ni, seed=12, zipf=True)
    got, ds, _ = _run(u, i, r, nu, ni, STAGED + [("runs_len", 4)], passes=1)
    assert ds.kind == 10 and ds.info(STAGE_STATE) == 1
    o = oracle.OracleTrainer("port", 0, 0)
    o.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64):
        o.set_param(kk, v)
    o.init_model()
    o.init_trainer()
    o.update_batch(sa.CSRData.from_triples(u, i, r))
    for name in NAMES:
        assert np.array_equal(got[name].view(np.uint32), o.view(name).view(np.uint32)), name

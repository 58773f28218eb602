"""`amd:step = auto` on the STAGED route of a one-GPU handle (svdf_staged.cpp): the decision is taken on the handle's
first chunk of at least device_schedule_min rows, from the chunk's exact level count and the estimator of the resident route (auto_step:
levels x unit latency against the bytes at the streaming rate), kept for the following chunks, re-taken after set_param, reported through
counters 16 .. 20.  Window chosen: the chunks train as under amd:step = minibatch.  Exact kept: the default step's bits."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from svdfeature_amd import CSRData

pytestmark = pytest.mark.gpu


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


def _bits(t, names):
    t.synchronize()
    return [t.view(n).copy().view(np.uint32) for n in names]


def _grouped_pairs(nu, ni, per_user, seed):
    """the generator's file order: a user's pairs are consecutive -- one dependency chain per user"""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(nu, dtype=np.uint32), per_user)
    p = rng.integers(0, ni, len(u)).astype(np.uint32)
    q = ((p + 1 + rng.integers(0, ni - 1, len(u))) % ni).astype(np.uint32)
    return sa.pairs_as_csr(u, p, q)


PAIR_VIEWS = ("W_user", "W_item", "i_bias")


def _pair_conf(nu, ni):
    return cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=64)


def test_a_deep_chunk_takes_the_window_step_and_the_minibatch_bits():
    nu, ni = 120, 400
    d = _grouped_pairs(nu, ni, 250, 7)
    knobs = [("device_schedule_min", 1000)]
    out = {}
    for step in ("auto", "minibatch", None):
        t = _trainer(_pair_conf(nu, ni), active=3, extra=[("amd:step", step)] if step else [], knobs=knobs)
        t.update_batch(d)
        t.finish_round()
        out[step] = _bits(t, PAIR_VIEWS)
        if step == "auto":
            assert t.counter(16) == 2 and t.counter(18) > 2 * t.counter(19) and t.counter(20) >= 1 and t.counter(17) >= 250 // 16
            assert t.counter(30) == 1 and t.counter(31) == 0
            # judged on the schedule the exact flush would build for this chunk: user-run units (svdf_punit.cpp), not one level per row
            x = _trainer(_pair_conf(nu, ni), active=3)
            dsx = x.dataset_from_pairs(d.feat_index[0::3], np.where(d.feat_value[1::3] > 0, d.feat_index[1::3], d.feat_index[2::3]),
                                       np.where(d.feat_value[1::3] > 0, d.feat_index[2::3], d.feat_index[1::3]))
            assert dsx.kind == 11 and t.counter(17) == dsx.num_batches
    assert all(np.array_equal(a, b) for a, b in zip(out["auto"], out["minibatch"]))
    assert any(not np.array_equal(a, b) for a, b in zip(out["auto"], out[None]))


def test_a_shallow_chunk_keeps_the_exact_step_and_the_default_bits():
    """uniform plain ratings, 2 M rows over 200 000 users x 60 000 items: a few dozen wide levels -- they stream, the exact step stays"""
    nu, ni, n = 200000, 60000, 2000000
    rng = np.random.default_rng(3)
    u = rng.integers(0, nu, n).astype(np.uint32)
    i = rng.integers(0, ni, n).astype(np.uint32)
    r = rng.integers(1, 6, n).astype(np.float32)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=64)
    names = ("W_user", "u_bias", "W_item", "i_bias")
    out = []
    for extra in ([("amd:step", "auto")], []):
        t = _trainer(conf, extra=extra)
        t.update_batch(d)
        t.finish_round()
        out.append(_bits(t, names))
        if extra:
            assert t.counter(16) == 1 and t.counter(18) <= 2 * t.counter(19) and 0 < t.counter(17) < 400
            assert t.counter(30) == 0 and t.counter(31) == 0
            launches = t.counter(1)
        else:
            assert t.counter(16) == 0 and t.counter(1) == launches
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_a_chunk_below_device_schedule_min_stays_exact_and_undecided():
    nu, ni = 120, 400
    d = _grouped_pairs(nu, ni, 50, 9)
    t = _trainer(_pair_conf(nu, ni), active=3, extra=[("amd:step", "auto")])   # device_schedule_min = 65 536 > 6 000 rows
    e = _trainer(_pair_conf(nu, ni), active=3)
    for x in (t, e):
        x.update_batch(d)
        x.finish_round()
    assert t.counter(16) == 0 and t.counter(30) == 0
    assert all(np.array_equal(a, b) for a, b in zip(_bits(t, PAIR_VIEWS), _bits(e, PAIR_VIEWS)))


def test_the_decision_is_kept_across_chunks_and_taken_again_after_set_param():
    nu, ni = 120, 400
    a, b = _grouped_pairs(nu, ni, 250, 7), _grouped_pairs(nu, ni, 100, 8)
    t = _trainer(_pair_conf(nu, ni), active=3, extra=[("amd:step", "auto")], knobs=[("device_schedule_min", 1000)])
    t.update_batch(a)
    t.finish_round()
    levels_a = t.counter(17)
    assert t.counter(16) == 2 and t.counter(30) == 1
    t.update_batch(b)
    t.finish_round()
    assert t.counter(30) == 2 and t.counter(17) == levels_a     # no new decision: the counters still describe chunk a
    tiny = a.slice_rows(0, 300)                                  # below device_schedule_min: the kept decision covers it too
    t.update_batch(tiny)
    t.finish_round()
    assert t.counter(30) == 3
    t.set_param("learning_rate", "0.004")
    t.update_batch(b)
    t.finish_round()
    assert t.counter(16) == 2 and t.counter(30) == 4 and 0 < t.counter(17) != levels_a   # decided again, on chunk b


def test_user_group_chunks_decide_from_their_unit_schedule(capfd):
    """SVD++ blocks: the decision comes from the exact unit schedule of the chunk (schedule_units on a scratch tracker); deep -> the closed units
    train as under amd:step = minibatch.  With lazy decay (outside the window step) the same chunks give decision 3, stay exact, and every
    one of them is counted and the rule is named once"""
    from svdfeature_amd import BlockArrays
    blocks = cases.user_blocks(400, 500, 150, 150, seed=6, max_rows=20, max_fb=12, split_every=3)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=500, num_item=150, num_factor=32, num_ufeedback=150, wd_ufeedback=0.004)
    names = ("W_user", "W_item", "W_ufeedback", "ufeedback_bias", "i_bias", "u_bias")
    out = {}
    for step in ("auto", "minibatch", None):
        t = sa.Trainer(1, 0)
        t.seed(10)
        for k, v in conf + ([("amd:step", step)] if step else []):
            t.set_param(k, str(v))
        t.init_model()
        t.init_trainer()
        t.set_knob("device_schedule_min", 500)
        for _ in range(2):
            for b in blocks:
                t.update_block(b)
            t.finish_round()
        out[step] = _bits(t, names)
        if step == "auto":
            assert t.counter(16) == 2 and t.counter(17) > 1 and t.counter(20) >= 1 and t.counter(30) == 2 and t.counter(31) == 0
            ex = sa.Trainer(1, 0)
            ex.seed(10)
            for k, v in conf:
                ex.set_param(k, str(v))
            ex.init_model()
            ex.init_trainer()
            assert t.counter(17) == ex.dataset_from_blocks(BlockArrays.from_blocks(blocks)).num_batches   # the exact schedule's levels
    assert all(np.array_equal(a, b) for a, b in zip(out["auto"], out["minibatch"]))
    assert any(not np.array_equal(a, b) for a, b in zip(out["auto"], out[None]))
    capfd.readouterr()
    lazy = cases.conf_with(conf, reg_method=4)
    got = []
    for step in ("auto", None):
        t = sa.Trainer(1, 0)
        t.seed(10)
        for k, v in lazy + ([("amd:step", step)] if step else []):
            t.set_param(k, str(v))
        t.init_model()
        t.init_trainer()
        t.set_knob("device_schedule_min", 500)
        for _ in range(2):
            for b in blocks:
                t.update_block(b)
            t.finish_round()
        got.append(_bits(t, names))
        if step:
            assert t.counter(16) == 3 and t.counter(30) == 0 and t.counter(31) == 2
    assert all(np.array_equal(a, b) for a, b in zip(*got))
    assert capfd.readouterr().err.count("keeps the exact") == 1

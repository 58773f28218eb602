"""The level kernels of the exact pass under every row-set count, block size, tile mapping and cache policy: k_basicmf,
k_basicmf_slots, k_fused, k_fewrow_fast and k_fewrow_slots through launch_basicmf / launch_fused, each knob combination against the sequential
oracle (`port`), trained once per (input, configuration, width).  Bit for bit on every parameter array after two passes and on
predict_dataset; there is no tolerance anywhere: the knobs never change a result.  Each combination first asserts, through the probe
svdf_level_geometry on the handle under test, the data set's kind and the launch counters, that it runs the form it claims; a knob the probe
reports as ignored is asserted as ignored.  The cases, inputs and the Python rule come from tests/level_geometry.py;
tests/test_level_geometry.py proves on the CPU that the inputs reach the edges of every launch shape run here."""
import numpy as np
import pytest

import level_geometry as lg
import svdfeature_amd as sa
from oracle import oracle

pytestmark = pytest.mark.gpu

PASSES = 2
VIEWS = ("W_user", "W_item", "u_bias", "i_bias", "g_bias")
BUILD_KNOBS = dict(use_fused=1, fewrow_gslots=1, pair_units=0, runs_exec=1, pivot_exec=1)   # what decides a data set's kind, set before it is built
_expected = {}


def _views(t):
    out = {}
    for name in VIEWS:
        v = t.view(name)
        if v is not None and v.size:
            out[name] = v.copy()
    return out


def expected(case):
    """the oracle's model after PASSES sequential passes over the input in file order, and its predictions on that model"""
    key = (case.input, case.conf, case.k)
    if key not in _expected:
        d = lg.make_input(case.input)
        o = lg.setup(oracle.OracleTrainer("port", 0, lg.CONFS[case.conf][0]), case.conf, case.k, d["ng"])
        first = _views(o)
        for _ in range(PASSES):
            o.update_batch(d["csr"])
        res = _views(o)
        assert any(not np.array_equal(res[name], first[name]) for name in res)
        _expected[key] = (first, res, o.predict_batch(d["csr"]))
        o.close()
    return _expected[key]


def chained_levels(widths, cap):
    """levels the engine hands to the chained launch: runs of four or more consecutive levels of at most `cap` instances"""
    total = run = 0
    for n in list(widths) + [cap + 1]:
        if cap > 0 and n <= cap:
            run += 1
        else:
            total += run if run >= 4 else 0
            run = 0
    return total


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        raise AssertionError("%s: %d of %d values differ in their bits, first at flat index %d: %r here, %r in the oracle"
                             % (what, bad.size, got.size, bad[0], float(got.ravel()[bad[0]]), float(want.ravel()[bad[0]])))


@pytest.mark.parametrize("case", lg.CASES, ids=[c.id for c in lg.CASES])
def test_every_knob_combination_trains_the_oracles_bits(case):
    d = lg.make_input(case.input)
    widths = [int(n) for n in d["widths"]]
    first, want, want_pred = expected(case)
    t = lg.setup(sa.Trainer(0, lg.CONFS[case.conf][0]), case.conf, case.k, d["ng"])
    for name, v in _views(t).items():          # both start from the same model
        same_bits(v, first[name], "initial " + name)
    for name, v in dict(BUILD_KNOBS, **{x: v for x, v in case.base.items() if x in BUILD_KNOBS}).items():
        t.set_knob(name, v)
    ds = {"triples": t.dataset_from_triples, "pairs": t.dataset_from_pairs}[d["kind"]](*d["cols"]) if d["kind"] != "rows" else t.dataset_from_csr(d["csr"])
    assert ds.kind == case.kind and ds.num_row == lg.N
    assert ds.num_batches == len(widths) and ds.max_batch == max(widths)            # the levels of the numpy rule
    launches = {0: 4, 1: 5, 2: 6}[case.kind]
    for combo in case.combos:
        knobs = dict(lg.DEFAULTS, **case.knobs(combo))
        for name, v in knobs.items():
            t.set_knob(name, v)
        # ---- the form this combination claims: the probe on this handle against the rule, for every level of the data set
        shapes = [case.probe(t, n) for n in widths]
        assert shapes == [case.rule(n, combo) for n in widths], combo
        if case.kind != 1:
            for name in lg.KNOBS:               # ignored means ignored: the launch does not move with a knob the form does not read
                if name not in shapes[0]["knobs"] and knobs[name] != lg.DEFAULTS[name]:
                    t.set_knob(name, lg.DEFAULTS[name])
                    assert [case.probe(t, n) for n in widths] == shapes, (combo, name)
                    t.set_knob(name, knobs[name])
        cap = shapes[0]["chain_cap"] if case.kind != 1 else 0
        chained = chained_levels(widths, cap)
        assert (chained > 0) == (case.name == "chained"), (combo, cap, chained)
        # ---- two passes from the initial model
        for name, v in first.items():
            t.set_view(name, v)
        before = {c: t.counter(c) for c in (4, 5, 6, 15)}
        for _ in range(PASSES):
            t.train_dataset(ds)
        got = _views(t)
        pred = t.predict_dataset(ds)
        after = {c: t.counter(c) for c in (4, 5, 6, 15)}
        # ---- the evidence of the route: the kind's launch counter moved by one per level and pass, the others not; the chained levels
        for c in (4, 5, 6):
            assert after[c] - before[c] == (PASSES * len(widths) if c == launches else 0), (combo, c)
        assert after[15] - before[15] == PASSES * chained, combo
        for name in want:
            same_bits(got[name], want[name], "%s %r: %s" % (case.id, combo, name))
        same_bits(pred, want_pred, "%s %r: predict_dataset" % (case.id, combo))
    ds.close()
    t.close()

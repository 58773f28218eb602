"""The exact schedule forms -- runs of an item's ratings (kind 10), hot rows walked as units (kind 9), user-run units of rank pairs (kind 11) and,
as the control, plain levels (kind 0) -- on ASYMMETRIC configurations (tests/forms_cases.py): the two sides' row decays, bias decays and the decayed
learning rate all differ, so a walker that swaps or drops one side's decay no longer computes the oracle's bits.  Every round the engine must equal
OracleTrainer("port") bit for bit -- parameters and predict_dataset --, eval_dataset to 1e-9 relative, on the route the case was written for."""
import numpy as np
import pytest

import forms_cases as fc
from oracle import oracle

pytestmark = pytest.mark.gpu


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check(case):
    import svdfeature_amd as sa
    oracle.build()
    data, (nu, ni) = fc.make_data(case)
    t = fc.setup(sa.Trainer(0, case["active"]), case, nu, ni)
    for k, v in case["knobs"]:
        t.set_knob(k, v)
    ds = t.dataset_from_pairs(*data[1:]) if data[0] == "pairs" else t.dataset_from_triples(*data[1:])
    assert ds.kind == case["kind"], (case["name"], ds.kind)
    csr = fc.as_csr(data)
    n = csr.num_row
    for r, o in fc.checker_rounds("port", case, data, nu, ni):
        t.set_round(r)
        t.train_dataset(ds)
        t.finish_round()
        got, want = fc.views(t), fc.views(o)
        for name in fc.NAMES:
            if got[name] is None or want[name] is None:
                continue
            assert _same(got[name], want[name]), (case["name"], "round", r, name)
        pg, po = t.predict_dataset(ds), o.predict_batch(csr)
        assert _same(pg, po), (case["name"], "round", r, "predict_dataset")
        ss, cnt = t.eval_dataset(ds)
        ref = oracle.sum_sq_err(po, csr.row_label)
        assert cnt == n and abs(ss - ref) <= 1e-9 * max(abs(ref), 1e-30), (case["name"], r, ss, ref)
    if case["kind"] in fc.COUNTER:
        assert t.counter(fc.COUNTER[case["kind"]]) == case["rounds"], case["name"]
    else:
        assert all(t.counter(c) == 0 for c in fc.COUNTER.values()), case["name"]
    ds.close()
    t.close()
    return want, data, nu, ni


def _mirrored_differs(case, direct, data, nu, ni):
    """non-vacuity: the oracle on the mirrored configuration (wd_user <-> wd_item, bias decays swapped) ends elsewhere, so the sizes and passes
    above are large enough to see a walker that uses one side's decays for the other"""
    for _, o in fc.checker_rounds("port", case, data, nu, ni, mirrored=True):
        pass
    mirrored = fc.views(o)
    for name in ("W_user", "W_item"):
        assert not _same(direct[name], mirrored[name]), (case["name"], name)


@pytest.mark.parametrize("case", fc.RUNS, ids=[c["name"] for c in fc.RUNS])
def test_runs_of_an_item_equal_the_oracle(case):
    direct, data, nu, ni = _check(case)
    if case is fc.RUNS[0]:
        _mirrored_differs(case, direct, data, nu, ni)


@pytest.mark.parametrize("case", fc.PIVOT, ids=[c["name"] for c in fc.PIVOT])
def test_hot_row_units_equal_the_oracle(case):
    direct, data, nu, ni = _check(case)
    if case is fc.PIVOT[0] or case is fc.PIVOT[1]:   # item-hot (transposed walker) and user-hot
        _mirrored_differs(case, direct, data, nu, ni)


@pytest.mark.parametrize("case", fc.PAIRS, ids=[c["name"] for c in fc.PAIRS])
def test_pair_units_equal_the_oracle(case):
    direct, data, nu, ni = _check(case)
    if case is fc.PAIRS[0]:
        _mirrored_differs(case, direct, data, nu, ni)


@pytest.mark.parametrize("case", fc.PLAIN, ids=[c["name"] for c in fc.PLAIN])
def test_plain_levels_equal_the_oracle(case):
    direct, data, nu, ni = _check(case)
    if case is fc.PLAIN[0]:
        _mirrored_differs(case, direct, data, nu, ni)

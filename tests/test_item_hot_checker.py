"""The item lane of the window step's checker on data rows (tests/window_sim.py: step_rows with isub), pinned on the CPU the way
tests/test_shared_hot_checker.py pins the user lane (whose helpers and fixture these tests use):
  * ONE sub-step that holds every slot of every item row (ihot_over = 0) is the plain window step bit for bit; with hot shared user rows in
    the same windows it is step_rows with the user lane alone;
  * a window in which one item id sits in every row -- as a plain entry, or as the feature_item child of every row's own item -- while every
    private user and every other item occurs once, in sub-steps of 1, moves the hot row like the port's sequential update_csr, up to the
    rounding of current + (new - current);
  * every checker run is the recorded one (tests/golden/window_checkers.npz)."""
import os

import numpy as np
import pytest

import window_sim as ws
from svdfeature_amd import CSRData
from test_shared_hot_checker import NI, NP, NS, _conf, _most_slots, _same, _table_case, _ub, case, run_case


P_ITEM_LANE = [(8, 0, ()), (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01"))), (5, 2, (("wd_item_bias", "0.02"),))]


@case(*P_ITEM_LANE)
def one_sub_step_for_every_slot_is_the_side_table_checker(S, tmp, k, reg, extra):
    conf, d, tu, ti, ub = _table_case(S, tmp, k, reg, extra, 50 + k)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, isub=d.num_row, fu=tu, fi=ti, user_bias=ub, ihot_over=0)
    b = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, fu=tu, fi=ti, user_bias=ub)
    return dict(a=a, b=b, conf=conf, d=d, ti=ti)


@pytest.mark.parametrize("k,reg,extra", P_ITEM_LANE)
def test_one_sub_step_for_every_slot_is_the_side_table_checker(request, k, reg, extra):
    out = run_case(request, (k, reg, extra))
    _same(out["a"], out["b"])
    assert not np.array_equal(out["b"].view("W_item")[NI - 1], ws.make_oracle(out["conf"]).view("W_item")[NI - 1])
    # a row of the lane that is both a plain entry and a child
    d, ti = out["d"], out["ti"]
    entries = {int(x) for r in range(d.num_row) for x in d.row(r)[4][d.row(r)[1] + d.row(r)[2]:]}
    assert entries & set(ws.children(ti, sorted(entries)))


P_BOTH_LANES = [(8, 0, (), 3), (16, 1, (("no_user_bias", "1"),), 1), (12, 3, (("wd_user_bias", "0.01"),), 5)]


@case(*P_BOTH_LANES)
def with_hot_user_rows_too_it_is_the_shared_hot_checker(S, tmp, k, reg, extra, sub):
    conf, d, tu, ti, ub = _table_case(S, tmp, k, reg, extra, 80 + k)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, isub=d.num_row, sub=sub, fu=tu, fi=ti, user_bias=ub, ihot_over=0)
    b = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, sub=sub, fu=tu, fi=ti, user_bias=ub)
    c = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, fu=tu, fi=ti, user_bias=ub)
    return dict(a=a, b=b, c=c, d=d, tu=tu, ti=ti)


@pytest.mark.parametrize("k,reg,extra,sub", P_BOTH_LANES)
def test_with_hot_user_rows_too_it_is_the_shared_hot_checker(request, k, reg, extra, sub):
    out = run_case(request, (k, reg, extra, sub))
    _same(out["a"], out["b"])
    assert _most_slots(out["d"], 2, NP, out["tu"], out["ti"])[0] > sub
    assert not np.array_equal(out["b"].view("W_user")[NP + 2], out["c"].view("W_user")[NP + 2])   # (the user lane did something in these windows)


@case(())
def a_sub_step_that_no_row_exceeds_changes_nothing(S, tmp):
    conf, d, tu, ti, ub = _table_case(S, tmp, 8, 0, (), 9)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1, isub=1000, fu=tu, fi=ti)
    b = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1, fu=tu, fi=ti)
    c = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1, isub=2, fu=tu, fi=ti)   # (a sub-step that hot rows do exceed: the record's only)
    return dict(a=a, b=b, c=c, d=d, tu=tu, ti=ti)


def test_a_sub_step_that_no_row_exceeds_changes_nothing(request):
    out = run_case(request, ())
    _same(out["a"], out["b"])
    assert _most_slots(out["d"], 3, NP, out["tu"], out["ti"])[1] > 2
    assert not np.array_equal(out["c"].view("W_item"), out["b"].view("W_item"))


P_ITEM_SEQ = [(8, 0, (), False), (7, 2, (("ip:wd", "0.01"), ("ip:bound", "10"), ("ip:wd", "0.002"), ("ip:bound", str(NI))), False),
              (16, 1, (("no_user_bias", "1"), ("wd_item_bias", "0.02")), True), (8, 3, (), True)]


@case(*P_ITEM_SEQ)
def sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(S, tmp, k, reg, extra, child):
    n, X = 20, NI - 1
    assert n <= NP and n < NI
    rng = np.random.default_rng(200 + k)
    users, items = rng.permutation(NP)[:n], rng.permutation(NI - 1)[:n]
    conf, ti = _conf(k, reg, extra), []
    if child:   # X is a child (value 0.5 or 2) of every item but itself
        path = S.write_table(os.path.join(tmp, "fi.txt"), [[(X, float(rng.choice([0.5, 2.0])))] for _ in range(NI - 1)])
        ti = S.read_table(path)
        conf = conf + [("feature_item", path)]
    rows = []
    for r in range(n):
        it = [(int(items[r]), float(rng.choice([1.0, 0.5, 1.25])))]
        if not child:
            it.append((X, float(rng.choice([1.0, 0.5, 2.0]))))
        rows.append((float(rng.integers(1, 6)), [], [(int(users[r]), 1.0)], it[::-1] if r % 2 else it))
    d = CSRData.from_rows(rows)
    B = NP + NS   # no shared user rows at all
    a = S.simulate_rows(S.make_oracle(conf), d, B, 1, 1, isub=1, fi=ti, user_bias=_ub(extra))
    # the plain window step: all n changes against the window-start row
    c = S.simulate_rows(S.make_oracle(conf), d, B, 1, 1, fu=(), fi=ti, user_bias=_ub(extra))
    return dict(a=a, c=c, conf=conf, d=d, X=X)


@pytest.mark.parametrize("k,reg,extra,child", P_ITEM_SEQ)
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(request, k, reg, extra, child):
    out = run_case(request, (k, reg, extra, child))
    a, c, d, X = out["a"], out["c"], out["d"], out["X"]
    b = ws.make_oracle(out["conf"])
    start = b.view("W_item")[X].copy()
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    np.testing.assert_allclose(a.view("W_item")[X], b.view("W_item")[X], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a.view("i_bias")[X], b.view("i_bias")[X], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(b.view("W_item")[X], start)
    # ... which the plain window step does not
    assert not np.allclose(c.view("W_item")[X], b.view("W_item")[X], rtol=1e-5, atol=1e-6)

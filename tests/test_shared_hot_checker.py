"""The checker of the window step on data rows (tests/window_sim.py: step_rows) without the item lane, pinned on the CPU from three sides; the item
lane's tests are tests/test_item_hot_checker.py, step_blocks' tests/test_block_item_hot_checker.py, and both use this module's helpers.

  * to what exists outside the checker: on rows with one user entry it is oracle update_batch_stale plus the window's add
    (multi_rank_utils.OracleShard) bit for bit; windows of one row, and sub-steps of 1 on a row that alone links its window's data rows, are the
    port's sequential update_csr within a stated float tolerance;
  * lane against walk: ONE sub-step that holds every slot of every shared row (hot_over = 0) is the plain window step, and a sub-step that no row
    exceeds changes nothing -- two argument settings of one function, bit for bit;
  * to tests/golden/window_checkers.npz: the final views of every checker run these three modules make, recorded from the seven single-purpose
    checker modules that window_sim replaced (one each for shared user rows, side tables, hot shared rows and hot item rows on data rows; for
    shared rows, hot shared rows and hot item rows on blocks), which the case functions were fed through an adapter with window_sim's
    interface.  Every case function takes the checker module S for that; the tests pass window_sim and must reproduce every recorded array
    bit for bit."""
import os

import numpy as np
import pytest

import cases
import window_sim as ws
from multi_rank_utils import OracleShard
from svdfeature_amd import CSRData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_checkers.npz")
NP, NS, NI, NG = 30, 20, 25, 6           # private users, shared users, items, globals
CASES = {}   # (module, test name) -> (case function, parameter sets): what the fixture holds, as "<module>::<test name>[<set>]/<side a, b, c>"


def case(*params):
    def deco(fn):
        CASES[fn.__module__.rsplit(".", 1)[-1], "test_" + fn.__name__] = (fn, list(params))
        return fn
    return deco


def flat_views(o):
    """all views of oracle trainer o, in window_sim.VIEWS' order, as one array: what the fixture holds per checker run"""
    return np.concatenate([o.view(v).ravel() for v in ws.VIEWS if o.view(v) is not None])


def run_case(request, params):
    """the requesting test's case at one of its parameter sets on window_sim: its checker runs must be the recorded ones"""
    name = request.node.module.__name__.rsplit(".", 1)[-1], request.node.originalname
    fn, sets = CASES[name]
    out = fn(ws, str(request.getfixturevalue("tmp_path")), *params)
    with np.load(GOLDEN) as g:
        sides = [s for s in "abc" if s in out]
        assert sides
        for s in sides:
            assert np.array_equal(flat_views(out[s]).view(np.uint32), g["%s::%s[%d]/%s" % (name + (sets.index(params), s))].view(np.uint32)), s
    return out


def _conf(k, reg, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


def _ub(extra):
    return dict(extra).get("no_user_bias", "0") != "1"


def _same(a, b, names=ws.SHARED):
    for name in names:
        x, y = a.view(name), b.view(name)
        if x is None or x.size == 0:
            continue
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


def _most_slots(d, W, B, fu=(), fi=()):
    """over the windows of d: the most slots one (shared user row, item row) has"""
    mu = mi = 0
    for b0, b1 in ws.row_cuts(d.num_row, W):
        win = d.slice_rows(b0, b1)
        users = [u for r in range(win.num_row) for u in ws.row_targets(win.row(r)[4], win.row(r)[1], win.row(r)[2], B, fu, fi)[0]]
        mu = max([mu] + [users.count(u) for u in set(users)])
        mi = max([mi] + list(ws.item_slot_counts(win, B, fu, fi).values()))
    return mu, mi




P_STALE = [(8, 0, 0, ()), (16, 2, 1, (("no_user_bias", "1"),)), (7, 0, 3, (("user_nonnegative", "1"),)),
           (5, 0, 2, (("up:wd", "0.01"), ("up:bound", "20"), ("up:wd", "0.002"), ("up:bound", "40")))]


@case(*P_STALE)
def checker_equals_the_stale_step_on_rows_with_one_user_entry(S, tmp, k, active, reg, extra):
    NU, NI, NG = 40, 30, 12
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NU, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)
    if active == 2:
        conf = cases.conf_with(conf, base_score="0.5")
    rng = np.random.default_rng(k)
    d = S.shared_rows(rng, 240, NU, 0, NI, num_global=NG, max_g=3, max_shared=0, uvals=True)
    if active == 2:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    a = S.make_oracle(conf, active=active)
    b = OracleShard(S.make_oracle(conf, active=active), minibatch=True)
    W = 4
    for _ in range(2):
        for b0, b1 in S.row_cuts(d.num_row, W):
            win = d.slice_rows(b0, b1)
            S.step_rows(a, win, NU, user_bias=_ub(extra))
            b.train(win)
            b.delta_set(b.delta_get())
    return dict(a=a, shard=b)


@pytest.mark.parametrize("k,active,reg,extra", P_STALE)
def test_checker_equals_the_stale_step_on_rows_with_one_user_entry(request, k, active, reg, extra):
    out = run_case(request, (k, active, reg, extra))
    for name in ("W_user", "u_bias", "W_item", "i_bias", "g_bias"):
        x, y = out["a"].view(name), out["shard"].t.view(name)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


P_EMPTY = [(8, 0, ()), (16, 1, (("no_user_bias", "1"),)), (5, 3, (("user_nonnegative", "1"),))]


@case(*P_EMPTY)
def empty_tables_give_the_shared_user_checker(S, tmp, k, reg, extra):
    fu = S.write_table(os.path.join(tmp, "fu.txt"), [[] for _ in range(NP + NS)])
    fi = S.write_table(os.path.join(tmp, "fi.txt"), [[] for _ in range(NI)])
    conf = _conf(k, reg, extra)
    rng = np.random.default_rng(k)
    d = S.table_rows(rng, 160, NP, NS, NI, num_global=NG, max_g=2, max_shared=3, max_items=2, uvals=True, ivals=True)
    a = S.make_oracle(conf + [("feature_user", fu), ("feature_item", fi)])
    b = S.make_oracle(conf)
    tu, ti = S.read_table(fu), S.read_table(fi)
    assert len(tu) == NP + NS and len(ti) == NI and not any(tu) and not any(ti)
    for _ in range(2):
        for b0, b1 in S.row_cuts(d.num_row, 3):
            win = d.slice_rows(b0, b1)
            S.step_rows(a, win, NP, fu=tu, fi=ti, user_bias=_ub(extra))
            S.step_rows(b, win, NP, user_bias=_ub(extra))
    return dict(a=a, b=b)


@pytest.mark.parametrize("k,reg,extra", P_EMPTY)
def test_empty_tables_give_the_shared_user_checker(request, k, reg, extra):
    out = run_case(request, (k, reg, extra))
    _same(out["a"], out["b"])


def test_table_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    rows = ws.random_table(rng, 40, NP, NP + NS, max_children=3, vals=(1.0, 0.1, 0.3, 2.5))
    got = ws.read_table(ws.write_table(str(tmp_path / "t.txt"), rows))
    assert got == [[(c, float(np.float32(v))) for c, v in r] for r in rows]
    assert all(NP <= c < NP + NS for r in got for c, _ in r)


P_ONE_ROW = [(8, 0, ()), (7, 2, (("up:wd", "0.01"), ("up:bound", "40"), ("up:wd", "0.002"), ("up:bound", str(NP + NS)))),
             (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01"), ("wd_user_bias", "0.02")))]


@case(*P_ONE_ROW)
def windows_of_one_row_are_the_sequential_pass(S, tmp, k, reg, extra):
    rng = np.random.default_rng(100 + k)
    tu = S.random_table(rng, NP + NS, NP, NP + NS, max_children=2)
    ti = S.random_table(rng, NI - 5, 0, NI, max_children=3)   # the last 5 item ids have no entry in the table
    fu = S.write_table(os.path.join(tmp, "fu.txt"), tu)
    fi = S.write_table(os.path.join(tmp, "fi.txt"), ti)
    tu, ti = S.read_table(fu), S.read_table(fi)
    conf = _conf(k, reg, extra) + [("feature_user", fu), ("feature_item", fi)]
    d = S.table_rows(rng, 90, NP, NS, NI, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = S.drop_rows_reaching_twice(d, NP, tu, ti)
    assert d.num_row > 40
    assert sum(len(S.children(ti, [int(x) for x in d.row(r)[4][d.row(r)[1] + d.row(r)[2]:]])) for r in range(d.num_row)) > 20
    a = S.simulate_rows(S.make_oracle(conf), d, NP, d.num_row, 1, fu=tu, fi=ti, user_bias=_ub(extra))
    return dict(a=a, conf=conf, d=d)


@pytest.mark.parametrize("k,reg,extra", P_ONE_ROW)
def test_windows_of_one_row_are_the_sequential_pass(request, k, reg, extra):
    out = run_case(request, (k, reg, extra))
    a, conf, d, ub = out["a"], out["conf"], out["d"], _ub(extra)
    b = ws.make_oracle(conf)
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    for name in ws.SHARED:
        x, y = a.view(name), b.view(name)
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6, err_msg=name)
        assert not np.array_equal(y, ws.make_oracle(conf).view(name)) or name == "u_bias" and not ub, name   # the pass moved it


P_USER_LANE = [(8, 0, ()), (16, 1, (("no_user_bias", "1"),)), (5, 3, (("user_nonnegative", "1"),)), (12, 2, (("wd_user_bias", "0.01"),))]


@case(*P_USER_LANE)
def one_sub_step_for_every_slot_is_the_shared_user_checker(S, tmp, k, reg, extra):
    conf = _conf(k, reg, extra)
    rng = np.random.default_rng(k)
    d = S.shared_rows(rng, 150, NP, NS, NI, num_global=NG, max_g=2, max_shared=3, uvals=True, hot=(NP, NP + 1), hot_p=0.6)
    a, b = S.make_oracle(conf), S.make_oracle(conf)
    for _ in range(2):
        for b0, b1 in S.row_cuts(d.num_row, 3):
            win = d.slice_rows(b0, b1)
            S.step_rows(a, win, NP, sub=win.num_row, user_bias=_ub(extra), hot_over=0)
            S.step_rows(b, win, NP, user_bias=_ub(extra))
    return dict(a=a, b=b, conf=conf, d=d)


@pytest.mark.parametrize("k,reg,extra", P_USER_LANE)
def test_one_sub_step_for_every_slot_is_the_shared_user_checker(request, k, reg, extra):
    out = run_case(request, (k, reg, extra))
    _same(out["a"], out["b"])
    assert _most_slots(out["d"], 3, NP)[0] > 0   # (the lane held rows)
    assert not np.array_equal(out["b"].view("W_user")[NP], ws.make_oracle(out["conf"]).view("W_user")[NP])


def _table_case(S, tmp, k, reg, extra, seed, item_hot=True):
    rng = np.random.default_rng(seed)
    tu = S.random_table(rng, NP + NS, NP, NP + NS, max_children=2, hot=(NP + 2,), hot_p=0.6)
    ti = S.random_table(rng, NI - 5, 0, NI, max_children=2, **(dict(hot=(NI - 1, NI - 2), hot_p=0.6) if item_hot else {}))
    fu, fi = S.write_table(os.path.join(tmp, "fu.txt"), tu), S.write_table(os.path.join(tmp, "fi.txt"), ti)
    tu, ti = S.read_table(fu), S.read_table(fi)
    conf = _conf(k, reg, extra) + [("feature_user", fu), ("feature_item", fi)]
    d = S.table_rows(rng, 120, NP, NS, NI, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = S.drop_rows_reaching_twice(d, NP, tu, ti)
    assert d.num_row > 50
    return conf, d, tu, ti, _ub(extra)


P_USER_LANE_TABLES = [(8, 0, ()), (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01")))]


@case(*P_USER_LANE_TABLES)
def one_sub_step_for_every_slot_is_the_side_table_checker(S, tmp, k, reg, extra):
    conf, d, tu, ti, ub = _table_case(S, tmp, k, reg, extra, 50 + k, item_hot=False)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, sub=d.num_row, fu=tu, fi=ti, user_bias=ub, hot_over=0)
    b = S.simulate_rows(S.make_oracle(conf), d, NP, 2, 2, fu=tu, fi=ti, user_bias=ub)
    return dict(a=a, b=b, d=d, tu=tu, ti=ti)


@pytest.mark.parametrize("k,reg,extra", P_USER_LANE_TABLES)
def test_one_sub_step_for_every_slot_is_the_side_table_checker(request, k, reg, extra):
    out = run_case(request, (k, reg, extra))
    _same(out["a"], out["b"])
    assert _most_slots(out["d"], 2, NP, out["tu"], out["ti"])[0] > 0


@case(())
def a_sub_step_that_no_row_exceeds_changes_nothing(S, tmp):
    conf = _conf(8, 0)
    rng = np.random.default_rng(9)
    d = S.shared_rows(rng, 90, NP, NS, NI, max_shared=2, hot=(NP,), hot_p=0.5)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1, sub=1000)
    b = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1)
    c = S.simulate_rows(S.make_oracle(conf), d, NP, 3, 1, sub=2)   # (a sub-step that the hot row does exceed: the record's only)
    return dict(a=a, b=b, c=c, d=d)


def test_a_sub_step_that_no_row_exceeds_changes_nothing(request):
    out = run_case(request, ())
    _same(out["a"], out["b"])
    assert _most_slots(out["d"], 3, NP)[0] > 2
    assert not np.array_equal(out["c"].view("W_user")[NP], out["b"].view("W_user")[NP])


P_USER_SEQ = [(8, 0, (), 0), (7, 2, (("up:wd", "0.01"), ("up:bound", "40"), ("up:wd", "0.002"), ("up:bound", str(NP + NS))), 1),
              (16, 1, (("no_user_bias", "1"), ("wd_user_bias", "0.02")), 1)]


@case(*P_USER_SEQ)
def sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(S, tmp, k, reg, extra, pos):
    n, X = 24, NP + 3
    assert n <= NP and n <= NI
    rng = np.random.default_rng(200 + k)
    users, items = rng.permutation(NP)[:n], rng.permutation(NI)[:n]
    rows = []
    for r in range(n):
        u = [(int(users[r]), 1.0), (X, float(rng.choice([1.0, 0.5, 2.0])))]
        rows.append((float(rng.integers(1, 6)), [], u if pos else u[::-1], [(int(items[r]), 1.0)]))
    d = CSRData.from_rows(rows)
    conf = _conf(k, reg, extra)
    a = S.simulate_rows(S.make_oracle(conf), d, NP, 1, 1, sub=1, user_bias=_ub(extra))
    # the plain window step: all n changes against the window-start row
    c = S.simulate_rows(S.make_oracle(conf), d, NP, 1, 1, user_bias=_ub(extra))
    return dict(a=a, c=c, conf=conf, d=d, X=X)


@pytest.mark.parametrize("k,reg,extra,pos", P_USER_SEQ)
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(request, k, reg, extra, pos):
    out = run_case(request, (k, reg, extra, pos))
    a, c, d, X = out["a"], out["c"], out["d"], out["X"]
    b = ws.make_oracle(out["conf"])
    start = b.view("W_user")[X].copy()
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    np.testing.assert_allclose(a.view("W_user")[X], b.view("W_user")[X], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a.view("u_bias")[X], b.view("u_bias")[X], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(b.view("W_user")[X], start)
    # ... which the plain window step does not
    assert not np.allclose(c.view("W_user")[X], b.view("W_user")[X], rtol=1e-5, atol=1e-6)

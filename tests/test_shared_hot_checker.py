"""The checker of the ordered sub-steps for hot shared user rows (tests/shared_hot_sim.py) pinned from two sides, CPU only:
  * ONE sub-step that holds every slot of every shared row (hot_over = 0: every shared row rides the lane) is the plain window step --
    shared_user_sim.window_step, and side_table_sim.window_step with tables -- bit for bit;
  * a window in which one shared id sits in every row while every private user and every item occurs once, in sub-steps of 1, moves the hot
    row like the reference's sequential update_inner (the port's update_csr), up to the rounding of current + (new - current): the float
    tolerance tests/test_side_table_checker.py uses for windows of one row."""
import numpy as np
import pytest

import cases
import shared_hot_sim as shs
import shared_user_sim
import side_table_sim as sts
from svdfeature_amd import CSRData

NP, NS, NI, NG = 30, 20, 25, 6
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def _conf(k, reg, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


@pytest.mark.parametrize("k,reg,extra", [(8, 0, ()), (16, 1, (("no_user_bias", "1"),)), (5, 3, (("user_nonnegative", "1"),)),
                                         (12, 2, (("wd_user_bias", "0.01"),))])
def test_one_sub_step_for_every_slot_is_the_shared_user_checker(k, reg, extra):
    conf = _conf(k, reg, extra)
    rng = np.random.default_rng(k)
    d = shared_user_sim.shared_rows(rng, 150, NP, NS, NI, num_global=NG, max_g=2, max_shared=3, uvals=True, hot=(NP, NP + 1), hot_p=0.6)
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a, b = shared_user_sim.make_oracle(conf), shared_user_sim.make_oracle(conf)
    for _ in range(2):
        for b0, b1 in shared_user_sim.window_cuts(d.num_row, 3):
            win = d.slice_rows(b0, b1)
            shs.window_step(a, win, NP, sub=win.num_row, user_bias=ub, hot_over=0)
            shared_user_sim.window_step(b, win, NP, ub)
    for name in VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name
    assert not np.array_equal(b.view("W_user")[NP], shared_user_sim.make_oracle(conf).view("W_user")[NP])


@pytest.mark.parametrize("k,reg,extra", [(8, 0, ()), (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01")))])
def test_one_sub_step_for_every_slot_is_the_side_table_checker(tmp_path, k, reg, extra):
    rng = np.random.default_rng(50 + k)
    tu = sts.random_table(rng, NP + NS, NP, NP + NS, max_children=2, hot=(NP + 2,), hot_p=0.6)
    ti = sts.random_table(rng, NI - 5, 0, NI, max_children=2)
    fu, fi = sts.write_table(str(tmp_path / "fu.txt"), tu), sts.write_table(str(tmp_path / "fi.txt"), ti)
    tu, ti = sts.read_table(fu), sts.read_table(fi)
    conf = _conf(k, reg, extra) + [("feature_user", fu), ("feature_item", fi)]
    d = sts.table_rows(rng, 120, NP, NS, NI, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = sts.drop_rows_reaching_twice(d, NP, tu, ti)
    assert d.num_row > 50
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a = shs.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, sub=d.num_row, fu=tu, fi=ti, user_bias=ub, hot_over=0)
    b = sts.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, tu, ti, ub)
    for name in VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name


def test_a_sub_step_that_no_row_exceeds_changes_nothing():
    conf = _conf(8, 0)
    rng = np.random.default_rng(9)
    d = shared_user_sim.shared_rows(rng, 90, NP, NS, NI, max_shared=2, hot=(NP,), hot_p=0.5)
    a = shs.simulate(shared_user_sim.make_oracle(conf), d, NP, 3, 1, sub=1000)
    b = shared_user_sim.simulate(shared_user_sim.make_oracle(conf), d, NP, 3, 1)
    for name in VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name


@pytest.mark.parametrize("k,reg,extra,pos", [(8, 0, (), 0), (7, 2, (("up:wd", "0.01"), ("up:bound", "40"), ("up:wd", "0.002"), ("up:bound", str(NP + NS))), 1),
                                             (16, 1, (("no_user_bias", "1"), ("wd_user_bias", "0.02")), 1)])
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(k, reg, extra, pos):
    n, S = 24, NP + 3
    assert n <= NP and n <= NI
    rng = np.random.default_rng(200 + k)
    users, items = rng.permutation(NP)[:n], rng.permutation(NI)[:n]
    rows = []
    for r in range(n):
        u = [(int(users[r]), 1.0), (S, float(rng.choice([1.0, 0.5, 2.0])))]
        rows.append((float(rng.integers(1, 6)), [], u if pos else u[::-1], [(int(items[r]), 1.0)]))
    d = CSRData.from_rows(rows)
    conf = _conf(k, reg, extra)
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a = shs.simulate(shared_user_sim.make_oracle(conf), d, NP, 1, 1, sub=1, user_bias=ub)
    b = shared_user_sim.make_oracle(conf)
    start = b.view("W_user")[S].copy()
    for r in range(n):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    np.testing.assert_allclose(a.view("W_user")[S], b.view("W_user")[S], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a.view("u_bias")[S], b.view("u_bias")[S], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(b.view("W_user")[S], start)
    # ... which the plain window step (all n changes against the window-start row) does not
    c = shared_user_sim.simulate(shared_user_sim.make_oracle(conf), d, NP, 1, 1, ub)
    assert not np.allclose(c.view("W_user")[S], b.view("W_user")[S], rtol=1e-5, atol=1e-6)

"""The checker of the ordered sub-steps for hot item rows (tests/item_hot_sim.py) pinned from two sides, CPU only:
  * ONE sub-step that holds every slot of every item row (ihot_over = 0: every item row rides the lane) is the plain window step --
    side_table_sim.window_step -- bit for bit; with hot shared user rows in the same windows it is shared_hot_sim.window_step bit for bit;
  * a window in which one item id sits in every row -- as a plain entry, or as the feature_item child of every row's own item -- while every
    private user and every other item occurs once, in sub-steps of 1, moves the hot row like the reference's sequential update_inner (the
    port's update_csr), up to the rounding of current + (new - current): the float tolerance tests/test_shared_hot_checker.py uses."""
import numpy as np
import pytest

import cases
import item_hot_sim as ihs
import shared_hot_sim as shs
import shared_user_sim
import side_table_sim as sts
from svdfeature_amd import CSRData

NP, NS, NI, NG = 30, 20, 25, 6
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def _conf(k, reg, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


def _same(a, b):
    for name in VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name


def _table_case(tmp_path, k, reg, extra, seed):
    rng = np.random.default_rng(seed)
    tu = sts.random_table(rng, NP + NS, NP, NP + NS, max_children=2, hot=(NP + 2,), hot_p=0.6)
    ti = sts.random_table(rng, NI - 5, 0, NI, max_children=2, hot=(NI - 1, NI - 2), hot_p=0.6)
    fu, fi = sts.write_table(str(tmp_path / "fu.txt"), tu), sts.write_table(str(tmp_path / "fi.txt"), ti)
    tu, ti = sts.read_table(fu), sts.read_table(fi)
    conf = _conf(k, reg, extra) + [("feature_user", fu), ("feature_item", fi)]
    d = sts.table_rows(rng, 120, NP, NS, NI, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = sts.drop_rows_reaching_twice(d, NP, tu, ti)
    assert d.num_row > 50
    return conf, d, tu, ti, dict(extra).get("no_user_bias", "0") != "1"


@pytest.mark.parametrize("k,reg,extra", [(8, 0, ()), (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01"))), (5, 2, (("wd_item_bias", "0.02"),))])
def test_one_sub_step_for_every_slot_is_the_side_table_checker(tmp_path, k, reg, extra):
    conf, d, tu, ti, ub = _table_case(tmp_path, k, reg, extra, 50 + k)
    a = ihs.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, isub=d.num_row, fu=tu, fi=ti, user_bias=ub, ihot_over=0)
    b = sts.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, tu, ti, ub)
    _same(a, b)
    assert not np.array_equal(b.view("W_item")[NI - 1], shared_user_sim.make_oracle(conf).view("W_item")[NI - 1])


@pytest.mark.parametrize("k,reg,extra,sub", [(8, 0, (), 3), (16, 1, (("no_user_bias", "1"),), 1), (12, 3, (("wd_user_bias", "0.01"),), 5)])
def test_with_hot_user_rows_too_it_is_the_shared_hot_checker(tmp_path, k, reg, extra, sub):
    conf, d, tu, ti, ub = _table_case(tmp_path, k, reg, extra, 80 + k)
    a = ihs.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, isub=d.num_row, sub=sub, fu=tu, fi=ti, user_bias=ub, ihot_over=0)
    b = shs.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, sub, tu, ti, ub)
    _same(a, b)
    c = sts.simulate(shared_user_sim.make_oracle(conf), d, NP, 2, 2, tu, ti, ub)   # (the user lane did something in these windows)
    assert not np.array_equal(b.view("W_user")[NP + 2], c.view("W_user")[NP + 2])


def test_a_sub_step_that_no_row_exceeds_changes_nothing(tmp_path):
    conf, d, tu, ti, ub = _table_case(tmp_path, 8, 0, (), 9)
    a = ihs.simulate(shared_user_sim.make_oracle(conf), d, NP, 3, 1, isub=1000, fu=tu, fi=ti)
    b = sts.simulate(shared_user_sim.make_oracle(conf), d, NP, 3, 1, tu, ti)
    _same(a, b)


@pytest.mark.parametrize("k,reg,extra,child", [(8, 0, (), False), (7, 2, (("ip:wd", "0.01"), ("ip:bound", "10"), ("ip:wd", "0.002"), ("ip:bound", str(NI))), False),
                                               (16, 1, (("no_user_bias", "1"), ("wd_item_bias", "0.02")), True), (8, 3, (), True)])
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(tmp_path, k, reg, extra, child):
    n, X = 20, NI - 1
    assert n <= NP and n < NI
    rng = np.random.default_rng(200 + k)
    users, items = rng.permutation(NP)[:n], rng.permutation(NI - 1)[:n]
    conf, ti = _conf(k, reg, extra), []
    if child:   # X is a child (value 0.5 or 2) of every item but itself
        ti = sts.read_table(sts.write_table(str(tmp_path / "fi.txt"), [[(X, float(rng.choice([0.5, 2.0])))] for _ in range(NI - 1)]))
        conf = conf + [("feature_item", str(tmp_path / "fi.txt"))]
    rows = []
    for r in range(n):
        it = [(int(items[r]), float(rng.choice([1.0, 0.5, 1.25])))]
        if not child:
            it.append((X, float(rng.choice([1.0, 0.5, 2.0]))))
        rows.append((float(rng.integers(1, 6)), [], [(int(users[r]), 1.0)], it[::-1] if r % 2 else it))
    d = CSRData.from_rows(rows)
    ub = dict(extra).get("no_user_bias", "0") != "1"
    B = NP + NS   # no shared user rows at all
    a = ihs.simulate(shared_user_sim.make_oracle(conf), d, B, 1, 1, isub=1, fi=ti, user_bias=ub)
    b = shared_user_sim.make_oracle(conf)
    start = b.view("W_item")[X].copy()
    for r in range(n):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    np.testing.assert_allclose(a.view("W_item")[X], b.view("W_item")[X], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(a.view("i_bias")[X], b.view("i_bias")[X], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(b.view("W_item")[X], start)
    # ... which the plain window step (all n changes against the window-start row) does not
    c = sts.simulate(shared_user_sim.make_oracle(conf), d, B, 1, 1, (), ti, ub)
    assert not np.allclose(c.view("W_item")[X], b.view("W_item")[X], rtol=1e-5, atol=1e-6)

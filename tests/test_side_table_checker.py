"""The checker of the window step with side tables (tests/side_table_sim.py) pinned from two sides, CPU only:
  * with tables that give no children it equals shared_user_sim.window_step (itself pinned to the stale-step checker) bit for bit;
  * with tables, windows of one row are the reference's sequential update_inner (the port's update_csr), up to the rounding of
    snapshot + (new - snapshot): within a stated float tolerance."""
import numpy as np
import pytest

import cases
import shared_user_sim
import side_table_sim as sts

NP, NS, NI, NG = 30, 20, 25, 6
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def _conf(k, reg, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


@pytest.mark.parametrize("k,reg,extra", [(8, 0, ()), (16, 1, (("no_user_bias", "1"),)), (5, 3, (("user_nonnegative", "1"),))])
def test_empty_tables_give_the_shared_user_checker(tmp_path, k, reg, extra):
    fu = sts.write_table(str(tmp_path / "fu.txt"), [[] for _ in range(NP + NS)])
    fi = sts.write_table(str(tmp_path / "fi.txt"), [[] for _ in range(NI)])
    conf = _conf(k, reg, extra)
    rng = np.random.default_rng(k)
    d = sts.table_rows(rng, 160, NP, NS, NI, num_global=NG, max_g=2, max_shared=3, max_items=2, uvals=True, ivals=True)
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a = shared_user_sim.make_oracle(conf + [("feature_user", fu), ("feature_item", fi)])
    b = shared_user_sim.make_oracle(conf)
    tu, ti = sts.read_table(fu), sts.read_table(fi)
    assert len(tu) == NP + NS and len(ti) == NI and not any(tu) and not any(ti)
    for _ in range(2):
        for b0, b1 in shared_user_sim.window_cuts(d.num_row, 3):
            win = d.slice_rows(b0, b1)
            sts.window_step(a, win, NP, tu, ti, ub)
            shared_user_sim.window_step(b, win, NP, ub)
    for name in VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name


def test_table_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    rows = sts.random_table(rng, 40, NP, NP + NS, max_children=3, vals=(1.0, 0.1, 0.3, 2.5))
    got = sts.read_table(sts.write_table(str(tmp_path / "t.txt"), rows))
    assert got == [[(c, float(np.float32(v))) for c, v in r] for r in rows]
    assert all(NP <= c < NP + NS for r in got for c, _ in r)


@pytest.mark.parametrize("k,reg,extra", [(8, 0, ()), (7, 2, (("up:wd", "0.01"), ("up:bound", "40"), ("up:wd", "0.002"), ("up:bound", str(NP + NS)))),
                                         (16, 3, (("no_user_bias", "1"), ("wd_item_bias", "0.01"), ("wd_user_bias", "0.02")))])
def test_windows_of_one_row_are_the_sequential_pass(tmp_path, k, reg, extra):
    rng = np.random.default_rng(100 + k)
    tu = sts.random_table(rng, NP + NS, NP, NP + NS, max_children=2)
    ti = sts.random_table(rng, NI - 5, 0, NI, max_children=3)   # the last 5 item ids have no entry in the table
    fu = sts.write_table(str(tmp_path / "fu.txt"), tu)
    fi = sts.write_table(str(tmp_path / "fi.txt"), ti)
    tu, ti = sts.read_table(fu), sts.read_table(fi)
    conf = _conf(k, reg, extra) + [("feature_user", fu), ("feature_item", fi)]
    d = sts.table_rows(rng, 90, NP, NS, NI, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True)
    d = sts.drop_rows_reaching_twice(d, NP, tu, ti)
    assert d.num_row > 40
    assert sum(len(sts.children(ti, [int(x) for x in d.row(r)[4][d.row(r)[1] + d.row(r)[2]:]])) for r in range(d.num_row)) > 20
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a = sts.simulate(shared_user_sim.make_oracle(conf), d, NP, d.num_row, 1, tu, ti, ub)
    b = shared_user_sim.make_oracle(conf)
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        b.update_csr(label, ng, nu, ni, idx, val)
    for name in VIEWS:
        x, y = a.view(name), b.view(name)
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6, err_msg=name)
        assert not np.array_equal(y, shared_user_sim.make_oracle(conf).view(name)) or name == "u_bias" and not ub, name   # the pass moved it

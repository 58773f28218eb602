"""Ordered sub-steps for hot shared user rows in the one-GPU window step (`amd:step = minibatch`, knobs `window_shared_sub` /
`window_shared_max`; svdf_wseq.cpp, svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_apply_shared).  A shared user row (id >=
amd:shared_user_from: a plain shared entry or a feature_user child) with more than window_shared_sub slots in a window is applied in file
order, that many slots at a time, every sub-step's changes formed against the row as the previous sub-step left it; everything else moves as
in the plain window step.  Every view must equal the checker of tests/window_sim.py -- the pinned C port driven one slot at a time --
bit for bit.  With the knob at 0 (the default) nothing changes."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import CSRData

pytestmark = pytest.mark.gpu

NP = 60                     # private users (B = NP)
NT, NA, NG = 40, 30, 6      # tracks, item attribute ids after them, global ids
NI = NT + NA
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


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


def _conf(k, ns, reg=0, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + ns, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


def _assert_same(t, o):
    for name in VIEWS:
        a, b = t.view(name), o.view(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def _slot_counts(d, b0, b1, B, fu=(), fi=()):
    c = {}
    for r in range(b0, b1):
        _, ng, nu, _, idx, _ = d.row(r)
        for u in ws.row_targets(idx, ng, nu, B, fu, fi)[0]:
            c[u] = c.get(u, 0) + 1
    return c


def _hot_per_row(d, B, window, sub, fu=(), fi=()):
    """(hot rows over all windows, the most hot entries one data row has, whether some hot row's slot count is no multiple of sub)"""
    nhot = most = 0
    ragged = False
    for b0 in range(0, d.num_row, window):
        b1 = min(b0 + window, d.num_row)
        c = _slot_counts(d, b0, b1, B, fu, fi)
        hot = {u for u, n in c.items() if n > sub}
        nhot += len(hot)
        ragged = ragged or any(c[u] % sub for u in hot)
        for r in range(b0, b1):
            _, ng, nu, _, idx, _ = d.row(r)
            most = max(most, sum(u in hot for u in ws.row_targets(idx, ng, nu, B, fu, fi)[0]))
    return nhot, most, ragged


def _up(ns):
    return (("up:wd", "0.01"), ("up:bound", str(NP + max(ns // 2, 1))), ("up:wd", "0.003"), ("up:bound", str(NP + ns)))


# (k, active_type, reg_method, extra keys, private positions, shared ids NS, window_shared_sub): NS = 4 makes every shared id hot and puts two
# or three hot entries into one data row; NS = 100 mixes three hot ids with rare ones
PLAIN = [
    (1, 0, 0, (), ("first",), 4, 1),
    (3, 0, 1, (("user_nonnegative", "1"),), ("last",), 4, 3),
    (7, 2, 3, (), ("middle",), 100, 5),
    (16, 3, 2, "up", ("first", "middle", "last"), 4, 12),
    (64, 0, 0, (), ("first", "middle", "last"), 100, 12),
    (64, 0, 1, (("no_user_bias", "1"),), ("first", "middle", "last"), 4, 7),
    (64, 2, 2, (("wd_user_bias", "0.01"),), ("middle", "last"), 100, 3),
    (100, 0, 3, "up", ("first", "middle", "last"), 4, 1),
    (128, 3, 0, (("no_user_bias", "1"), ("wd_user_bias", "0.01")), ("first", "last"), 100, 1),
    (200, 0, 2, (("user_nonnegative", "1"),), ("first", "middle", "last"), 4, 12),
    (256, 0, 1, "up", ("first", "middle", "last"), 100, 5),
    (256, 2, 0, (("wd_user_bias", "0.005"), ("wd_item_bias", "0.01")), ("middle",), 4, 3),
]


@pytest.mark.parametrize("k,active,reg,extra,positions,ns,sub", PLAIN)
def test_hot_shared_rows_in_sub_steps_equal_the_checker(k, active, reg, extra, positions, ns, sub):
    extra = _up(ns) if extra == "up" else extra
    conf = cases.conf_with(_conf(k, ns, reg, extra), active_type=active)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    rng = np.random.default_rng(1000 + k + reg)
    hot = (NP, NP + 1, NP + 2)
    d = ws.shared_rows(rng, 330, NP, ns, NT, num_global=NG, max_g=2, max_shared=3, uvals=True, hot=hot, hot_p=0.8,
                                    positions=positions)
    if active != 0:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    nhot, most, ragged = _hot_per_row(d, NP, 90, sub)
    assert nhot >= 8 and (most >= 2 or ns > 4) and (ragged or sub == 1)
    t = _trainer(conf, active, [("amd:step", "minibatch"), ("amd:window", 90), ("amd:shared_user_from", NP)], [("window_shared_sub", sub)])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8
    W = ds.num_batches
    assert W == (d.num_row + 89) // 90   # with amd:window the window size is the caller's
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    ub = dict(extra).get("no_user_bias") != "1"
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, NP, W, 2, sub=sub, user_bias=ub)
    _assert_same(t, o)
    # the lane did something: the plain window step ends elsewhere
    p = ws.simulate_rows(ws.make_oracle(conf, active=active), d, NP, W, 2, user_bias=ub)
    assert not np.array_equal(p.view("W_user")[NP], o.view("W_user")[NP])


def _tables(tmp_path, seed, which, ns):
    rng = np.random.default_rng(seed)
    hot = (NP, NP + 1)
    tu = ws.read_table(ws.write_table(str(tmp_path / "fu.txt"), ws.random_table(rng, NP + ns, NP, NP + ns, 2, hot=hot, hot_p=0.7)))
    keys, ti = [("feature_user", str(tmp_path / "fu.txt"))], []
    if which == "both":
        ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), ws.random_table(rng, NT, NT, NI, 3, hot=(NT, NT + 1), hot_p=0.7)))
        keys.append(("feature_item", str(tmp_path / "fi.txt")))
    return keys, tu, ti


# (k, active_type, reg_method, extra keys, private positions, tables, window_shared_sub): the table gives every user id -- private users AND
# shared entries -- up to two children among the shared ids, two of them hot
TABLES = [
    (5, 0, 0, (), ("first",), "user", 1),
    (16, 2, 3, (), ("last",), "both", 3),
    (64, 0, 0, (), ("first", "middle", "last"), "both", 3),
    (64, 3, 1, (("no_user_bias", "1"),), ("first", "middle", "last"), "both", 12),
    (128, 0, 2, "up", ("first", "middle", "last"), "both", 5),
    (256, 0, 3, (("user_nonnegative", "1"), ("wd_user_bias", "0.005")), ("middle", "last"), "user", 1),
]


@pytest.mark.parametrize("k,active,reg,extra,positions,which,sub", TABLES)
def test_hot_feature_user_children_in_sub_steps_equal_the_checker(tmp_path, k, active, reg, extra, positions, which, sub):
    ns = 100
    extra = _up(ns) if extra == "up" else extra
    keys, tu, ti = _tables(tmp_path, k + reg, which, ns)
    conf = cases.conf_with(_conf(k, ns, reg, extra), active_type=active) + keys
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    rng = np.random.default_rng(k + reg)
    d = ws.table_rows(rng, 360, NP, ns, NT, num_global=NG, max_g=2, max_shared=2, max_items=2, uvals=True, ivals=True, positions=positions)
    d = ws.drop_rows_reaching_twice(d, NP, tu, ti)
    if active != 0:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    nhot, most, _ = _hot_per_row(d, NP, 90, sub, tu, ti)
    assert d.num_row > 150 and nhot >= 4 and most >= 2   # hot children of the private user and of a shared entry in one data row
    t = _trainer(conf, active, [("amd:step", "minibatch"), ("amd:window", 90), ("amd:shared_user_from", NP)], [("window_shared_sub", sub)])
    ds = t.dataset_from_csr(d)
    W = ds.num_batches
    assert ds.kind == 8 and W == (d.num_row + 89) // 90
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    ub = dict(extra).get("no_user_bias") != "1"
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, NP, W, 2, sub=sub, fu=tu, fi=ti, user_bias=ub)
    _assert_same(t, o)
    p = ws.simulate_rows(ws.make_oracle(conf, active=active), d, NP, W, 2, fu=tu, fi=ti, user_bias=ub)
    assert not np.array_equal(p.view("W_user")[NP], o.view("W_user")[NP])


def _deep_rows(n, seed):
    """300 private users, 4 shared ids met by every row (n / 4 each), 8 global ids, 200 items: the shape of
    tests/test_gpu_shared_user_window.py::test_default_window_rule_keeps_shared_rows_at_12_updates_per_window"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        u = int(rng.integers(0, 300))
        rows.append((float(rng.integers(1, 6)), [(int(rng.integers(0, 8)), float(rng.uniform(0.1, 1.0)))], [(u, 1.0), (300 + u % 4, 1.0)],
                     [(int(rng.integers(0, 200)), 1.0)]))
    return CSRData.from_rows(rows)


DEEP_CONF = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=200, num_global=8, num_factor=32, wd_global="0.001")


def test_knob_at_zero_is_the_knob_unset():
    """the default rule, the same windows and the same bits; and the lane, once switched on, is what moves the result"""
    d = _deep_rows(6000, 3)
    got = []
    for knobs in ((), (("window_shared_sub", 0),), (("window_shared_sub", 0), ("window_shared_max", 32)), (("window_shared_sub", 12),)):
        t = _trainer(DEEP_CONF, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)], knobs=knobs)
        ds = t.dataset_from_csr(d)
        for _ in range(2):
            t.train_dataset(ds)
        t.synchronize()
        got.append((ds.kind, ds.num_batches, {name: t.view(name).copy() for name in VIEWS}))
    uid = d.feat_index[d.row_ptr[1:-1:3] + 1].astype(np.int64)
    W0 = int(np.ceil(wr.met(np.bincount(uid - 300, minlength=4), 12 / 128) / 12))   # about 1 500 updates per shared row at 12 per window
    assert got[0][:2] == got[1][:2] == got[2][:2] == (8, W0)
    for other in got[1:3]:
        for name in VIEWS:
            assert np.array_equal(got[0][2][name].view(np.uint32), other[2][name].view(np.uint32)), name
    assert got[3][1] < W0 and not np.array_equal(got[0][2]["W_user"][300:], got[3][2]["W_user"][300:])


def test_window_rule_with_sub_steps():
    d = _deep_rows(20000, 3)
    uid = d.feat_index[d.row_ptr[1:-1:3] + 1].astype(np.int64)
    shared = np.bincount(uid - 300, minlength=4)
    items = np.bincount(d.feat_index[d.row_ptr[2:-1:3]].astype(np.int64), minlength=200)
    globs = np.bincount(d.feat_index[d.row_ptr[0:-1:3]].astype(np.int64), minlength=8)
    assert shared.sum() == items.sum() == globs.sum() == 20000
    t = _trainer(DEEP_CONF, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)])
    default = t.dataset_from_csr(d).num_batches
    assert default == int(np.ceil(wr.met(shared, 12 / 128) / 12)) == wr.csr(20000, items, globs, shared)
    t.set_knob("window_per_target", 100000)   # (the global biases out of the way: 8 ids met by 2 500 rows each ask for 105 windows of their own)
    assert t.dataset_from_csr(d).num_batches == default
    for sub, cap in ((12, 256), (12, 64), (3, 1024), (8, 512)):
        t.set_knob("window_shared_sub", sub)
        t.set_knob("window_shared_max", cap)
        W = t.dataset_from_csr(d).num_batches
        assert W == wr.csr(20000, items, globs, shared, shared_lane=(sub, cap), per_target=100000), (sub, cap)
        assert W < default
    # sub-steps larger than the class mean: the mean term binds (16 of 16 -> c / W <= 12 again)
    t.set_knob("window_shared_sub", 16)
    t.set_knob("window_shared_max", 512)
    assert t.dataset_from_csr(d).num_batches == wr.csr(20000, items, globs, shared, shared_lane=(16, 512), per_target=100000) == default
    t.set_knob("window_per_target", 24)
    t.set_knob("window_shared_sub", 12)
    t.set_knob("window_shared_max", 128)
    W = t.dataset_from_csr(d).num_batches
    assert W == wr.csr(20000, items, globs, shared, shared_lane=(12, 128)) and W < default


def test_train_dataset_refuses_a_knob_changed_since_the_build():
    d = _deep_rows(3000, 5)
    t = _trainer(DEEP_CONF, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)], knobs=[("window_shared_sub", 12)])
    ds = t.dataset_from_csr(d)
    t.train_dataset(ds)
    for other in (3, 0):
        t.set_knob("window_shared_sub", other)
        with pytest.raises(sa.SvdfError, match="built with another window_shared_sub"):
            t.train_dataset(ds)
    t.set_knob("window_shared_sub", 12)
    t.train_dataset(ds)
    t.synchronize()
    with pytest.raises(sa.SvdfError, match=r"window_shared_sub must be in 0 \.\. 4096"):
        t.set_knob("window_shared_sub", -1)
    with pytest.raises(sa.SvdfError, match="window_shared_max must be positive"):
        t.set_knob("window_shared_max", 0)


def test_refusals_name_their_cause():
    one = CSRData.from_rows([(3.0, [], [(0, 1.0), (NP + 1, 1.0)], [(2, 1.0)])])
    mb = [("amd:step", "minibatch"), ("amd:shared_user_from", NP)]
    # bf16 contribution rows
    t = _trainer(_conf(8, 10), 0, mb + [("amd:contrib", "bf16")], [("window_shared_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"window_shared_sub > 0 \(ordered sub-steps for hot shared user rows\) needs amd:contrib = fp32"):
        t.dataset_from_csr(one)
    # the N-rank window builder
    t = _trainer(_conf(8, 10), 0, [], [("window_shared_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"svdf_dataset_window_from_csr: window_shared_sub > 0 .* is for the one-GPU window sequence"):
        t.dataset_window_from_csr(CSRData.from_rows([(3.0, [], [(0, 1.0)], [(2, 1.0)])]))
    # user-group (SVD++) trainers
    blocks = cases.user_blocks(6, 20, NT, NT, seed=2)
    g = sa.Trainer(1, 0)
    g.seed(10)
    for k_, v_ in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=NI, num_factor=8, num_ufeedback=NT) + [("amd:step", "minibatch")]:
        g.set_param(k_, str(v_))
    g.init_model()
    g.init_trainer()
    g.set_knob("window_shared_sub", 12)
    with pytest.raises(sa.SvdfError, match=r"window_shared_sub > 0 .* is not supported with user-group \(SVD\+\+\) trainers"):
        g.dataset_from_blocks(blocks)
    g.set_knob("window_shared_sub", 0)
    g.dataset_from_blocks(blocks).close()


def test_short_fuzz_run():
    import fuzz_shared_hot
    assert fuzz_shared_hot.run(iters=12, seed=7) == 0

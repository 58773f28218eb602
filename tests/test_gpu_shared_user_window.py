"""Shared user rows in the one-GPU window step (`amd:shared_user_from = B`; svdf_wunit.cpp, svdf_k_wunit.hip): user ids
< B are private (one per row, walked exactly by its unit), ids >= B are shared attribute rows (an age bucket, a region ...) read as of the
window start and moved once per window, like item rows.  Every view must equal the checker of tests/window_sim.py -- the pinned C port
of the reference's update_inner (apex_svd_base.h:456-462) row by row on (the private user's current row, the window-start shared rows),
shared changes summed per target in file order -- bit for bit."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import CSRData

pytestmark = pytest.mark.gpu

NP, NS, NI, NG = 60, 200, 40, 8      # private users, shared user ids (B = NP), items, global ids
HOT = (NP, NP + 1)                   # two very hot shared ids: many slots per window; the other 198 mostly meet one row (in-place applies)
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def _trainer(conf, active=0, extra=()):
    t = sa.Trainer(0, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    return t


def _conf(k, reg=0, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)


def _data(seed, n=360, positions=("first", "middle", "last"), binary=False):
    rng = np.random.default_rng(seed)
    d = ws.shared_rows(rng, n, NP, NS, NI, num_global=NG, max_g=2, max_shared=3, uvals=True, hot=HOT, hot_p=0.7,
                                    positions=positions)
    if binary:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    return d


def _assert_same(t, o):
    for name in VIEWS:
        a, b = t.view(name), o.view(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


CASES = [  # (k, active_type, reg_method, extra keys, private positions)
    (1, 0, 0, (), ("first",)),
    (7, 0, 1, (("user_nonnegative", "1"),), ("middle",)),
    (16, 2, 3, (), ("last",)),
    (64, 0, 0, (), ("first", "middle", "last")),
    (64, 3, 1, (("no_user_bias", "1"),), ("first", "middle", "last")),
    (128, 0, 2, (("up:wd", "0.01"), ("up:bound", "100"), ("up:wd", "0.003"), ("up:bound", str(NP + NS))), ("first", "middle", "last")),
    (128, 2, 0, (("no_user_bias", "1"), ("wd_user_bias", "0.01")), ("middle", "last")),
    (256, 0, 3, (("up:wd", "0.002"), ("up:bound", "30"), ("up:wd", "0.02"), ("up:bound", str(NP + NS))), ("first", "last")),
    (256, 3, 2, (), ("first", "middle", "last")),
]


@pytest.mark.parametrize("k,active,reg,extra,positions", CASES)
def test_minibatch_with_shared_user_rows_equals_the_checker(k, active, reg, extra, positions):
    conf = cases.conf_with(_conf(k, reg, extra), active_type=active)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    d = _data(k + reg, positions=positions, binary=active != 0)
    t = _trainer(conf, active, [("amd:step", "minibatch"), ("amd:window", 90), ("amd:shared_user_from", NP)])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8
    W = ds.num_batches
    assert W == 4
    for _ in range(3):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, NP, W, 3, user_bias=dict(extra).get("no_user_bias") != "1")
    _assert_same(t, o)


def _deep_rows(n, seed, shared=True):
    """300 private users, 4 shared ids met by every row (n / 4 each: the exact levels are n / 4 deep), 8 global ids"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        u = int(rng.integers(0, 300))
        users = [(u, 1.0)] + ([(300 + u % 4, 1.0)] if shared else [])
        rows.append((float(rng.integers(1, 6)), [(int(rng.integers(0, 8)), float(rng.uniform(0.1, 1.0)))], users, [(int(rng.integers(0, 200)), 1.0)]))
    return CSRData.from_rows(rows)


def test_auto_takes_the_window_step_with_the_key_and_keeps_exact_levels_without():
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=200, num_global=8, num_factor=32, wd_global="0.001")
    d = _deep_rows(20000, 3)
    t = _trainer(conf, extra=[("amd:step", "auto"), ("amd:shared_user_from", 300)])
    ds = t.dataset_from_csr(d)
    assert t.counter(16) == 2 and ds.kind == 8
    m = _trainer(conf, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)])
    dm = m.dataset_from_csr(d)
    assert dm.num_batches == ds.num_batches
    for _ in range(2):
        t.train_dataset(ds)
        m.train_dataset(dm)
    t.synchronize(); m.synchronize()
    _assert_same(t, m)
    e = _trainer(conf, extra=[("amd:step", "auto")])   # without the key: what the engine does today
    de = e.dataset_from_csr(d)
    assert e.counter(16) == 3 and de.kind != 8


@pytest.mark.parametrize("k", [16, 64])
def test_the_key_on_data_without_shared_ids_changes_nothing(k):
    conf = _conf(k)
    d = _data(5, positions=("first",))
    keep = np.ones(d.num_row, bool)
    for r in range(d.num_row):
        keep[r] = d.row(r)[2] == 1
    d = d.select_rows(keep)
    got = []
    for extra in ([], [("amd:shared_user_from", NP)]):
        t = _trainer(conf, 0, [("amd:step", "minibatch"), ("amd:window", 60)] + extra)
        ds = t.dataset_from_csr(d)
        for _ in range(3):
            t.train_dataset(ds)
        t.synchronize()
        got.append({name: t.view(name).copy() for name in VIEWS})
    for name in VIEWS:
        assert np.array_equal(got[0][name].view(np.uint32), got[1][name].view(np.uint32)), name


def test_refusals_name_their_cause():
    conf = _conf(8)
    mb = [("amd:step", "minibatch"), ("amd:shared_user_from", NP)]
    t = _trainer(conf, 0, mb)
    two_private = CSRData.from_rows([(3.0, [], [(1, 1.0), (2, 1.0)], [(2, 1.0)])])
    with pytest.raises(sa.SvdfError, match="exactly one private user entry.*two"):
        t.dataset_from_csr(two_private)
    with pytest.raises(sa.SvdfError, match="exactly one private user entry.*none"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(NP + 3, 1.0)], [(2, 1.0)])]))
    with pytest.raises(sa.SvdfError, match="shared user id listed twice"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(1, 1.0), (NP + 3, 1.0), (NP + 3, 0.5)], [(2, 1.0)])]))
    shared = CSRData.from_rows([(3.0, [], [(1, 1.0), (NP + 3, 1.0)], [(2, 1.0)])])
    b = _trainer(conf, 0, mb + [("amd:contrib", "bf16")])
    with pytest.raises(sa.SvdfError, match="amd:contrib = fp32"):
        b.dataset_from_csr(shared)
    w = _trainer(conf, 0, [("amd:shared_user_from", NP)])
    with pytest.raises(sa.SvdfError, match="N-rank"):
        w.dataset_window_from_csr(shared)
    # without the key the message stays the one of today
    p = _trainer(conf, 0, [("amd:step", "minibatch")])
    with pytest.raises(sa.SvdfError, match="exactly one user"):
        p.dataset_from_csr(shared)
    g = sa.Trainer(0, 0)
    g.set_param("amd:gpus", "2")
    with pytest.raises(sa.SvdfError, match="one GPU only"):
        g.set_param("amd:shared_user_from", str(NP))
    h = sa.Trainer(0, 0)
    h.set_param("amd:shared_user_from", str(NP))
    with pytest.raises(sa.SvdfError, match="one GPU only"):
        h.set_param("amd:gpus", "2")
    # 1 <= B <= num_user: checked when the key is parsed once the model's shape is known, else by init_trainer
    x = _trainer(conf, 0, [("amd:step", "minibatch")])
    for bad in ("0", str(NP + NS + 1)):
        with pytest.raises(sa.SvdfError, match=r"amd:shared_user_from must be in 1 \.\. num_user"):
            x.set_param("amd:shared_user_from", bad)
    y = sa.Trainer(0, 0)
    for k_, v_ in conf + [("amd:shared_user_from", str(NP + NS + 1))]:
        y.set_param(k_, str(v_))
    y.init_model()
    with pytest.raises(sa.SvdfError, match=r"amd:shared_user_from must be in 1 \.\. num_user"):
        y.init_trainer()


def test_auto_keeps_exact_levels_where_the_window_step_would_refuse_the_shared_rows():
    """bf16 contribution rows are refused with shared entries: `auto` must see the rows as not covered (decision 3), not fail"""
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=200, num_global=8, num_factor=32, wd_global="0.001")
    d = _deep_rows(20000, 3)
    t = _trainer(conf, extra=[("amd:step", "auto"), ("amd:shared_user_from", 300), ("amd:contrib", "bf16")])
    ds = t.dataset_from_csr(d)
    assert t.counter(16) == 3 and ds.kind != 8
    t.train_dataset(ds)
    e = _trainer(conf)
    de = e.dataset_from_csr(d)
    e.train_dataset(de)
    t.synchronize(); e.synchronize()
    _assert_same(t, e)   # the exact pass, as without the key


def test_default_window_rule_keeps_shared_rows_at_12_updates_per_window():
    """4 shared ids met by 5 000 rows each (global ids 2 500, items ~100): the shared rows set the window count, at 12 per window by default
    (window_per_target_shared) -- not at the 24 of item rows, which misses the accuracy contract on the SURVEY 8(d2) variant"""
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=200, num_global=8, num_factor=32, wd_global="0.001")
    d = _deep_rows(20000, 3)
    counts = np.bincount(d.feat_index[d.row_ptr[1:-1:3] + 1] - 300, minlength=4)
    met = wr.met(counts, 0.0)   # updates an entry's shared row meets per pass: sum c^2 / sum c (the most updates of one row do not bind here)
    t = _trainer(conf, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)])
    assert t.dataset_from_csr(d).num_batches == int(np.ceil(met / 12))
    t.set_knob("window_per_target_shared", 24)
    assert t.dataset_from_csr(d).num_batches == int(np.ceil(met / 24))


def test_short_fuzz_run():
    import fuzz_shared_user
    assert fuzz_shared_user.run(iters=12, seed=7) == 0

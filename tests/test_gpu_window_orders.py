"""The one-GPU window sequence (`amd:step = minibatch / auto`) on clustered file orders (tests/window_order_cases.py; svdf_wseq_rule.h:
wseq_actual_columns / wseq_actual_csr; knob `window_count_actual`).  The window rule is evaluated on the windows as they
are cut, so that what include/svdfeature_amd.h states about a window -- the mean over entries of min(count, sub) at the class's per-target value,
no row more than the class's cap, both times the slack 1.5 -- holds on a file sorted by item, one that arrives in bursts, one sorted by a shared
user id, as it does on a shuffled one:

  a  the documented bounds hold on the windows as cut (triples, rank pairs, rows with shared user ids; lanes on and off; every order)
  b  the kernels equal the checkers bit for bit on the many small windows clustered files produce
  c  the accuracy contract |dRMSE| <= 1e-4 against the exact pass on the burst order
  d  `amd:step = auto` on the item order: the exact pass, or a sequence that satisfies a and c
  e  shuffled files keep their windows and their bits (window_count_actual 1 against 0)
  f  window_count_actual = 0 is the per-pass rule of before (build only: that configuration ends in NaN on these files and is never trained)
  g  window_hot_sub is recorded at build: train_dataset refuses a sequence built with another value

(The block sequence, wseq_from_blocks, is not covered: its windows keep the per-pass rule.)"""
import numpy as np
import pytest

import cases
import pair_hot_cases as ph
import window_order_cases as woc
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from test_window_orders import CONTRACT, HOT_MAX, HOT_SUB, K, N, NI, NU, PARENT_W, PER, PER_MAX, SEED, SLACK

pytestmark = pytest.mark.gpu

MB = [("amd:step", "minibatch")]
NAMES = ("W_item", "i_bias", "W_user", "u_bias")
PER_SHARED, SHARED_MAX, ITEM_MAX, PAIR_MAX = 12, 512, 2048, 4096   # window_per_target_shared, window_shared_max, window_item_max, window_pair_max
AN, ANU, ANI = 60000, 6000, 150                                   # the sizes of (a), (b), (e): 400 ratings per item


def _trainer(conf, extra=(), knobs=(), active=None):
    active = int(dict(conf).get("active_type", 0)) if active is None else active
    t = sa.Trainer(0, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _conf(nu, ni, k):
    return cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)


def _pair_conf(nu, ni, k):
    return cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k)


def _bounds(cols, num_id, W, sub, cap, per=PER):
    """the two quantities of the rule on the windows as cut, asserted at what the engine enforces (the header's value times the slack)"""
    worst, per_entry = woc.window_counts(cols, num_id, W)
    mean = woc.mean_met(per_entry, sub)
    assert worst <= cap * SLACK, ("worst count per window", worst, cap, W)
    assert mean <= per * SLACK, ("mean over entries of min(count, sub)", mean, per, W)
    return worst, mean


def _views(t, names=NAMES):
    t.synchronize()
    return {nm: t.view(nm).copy() for nm in names}


def _same(a, b, what=()):
    for nm in a:
        assert np.array_equal(a[nm].view(np.uint32), b[nm].view(np.uint32)), (nm,) + tuple(what)


# ------------------------------------------------------------------------------------------------ a: the documented bounds
@pytest.mark.parametrize("order", woc.ORDERS)
@pytest.mark.parametrize("sub", [HOT_SUB, 0])
def test_a_triples_windows_keep_the_documented_bounds(order, sub):
    u, i, r = woc.triples(AN, ANU, ANI, SEED, order)
    t = _trainer(_conf(ANU, ANI, 16), MB, [("window_hot_sub", sub)])
    ds = t.dataset_from_triples(u, i, r)
    W = ds.num_batches
    assert ds.kind == 8
    _bounds(i, ANI, W, sub, HOT_MAX if sub else PER_MAX)
    W0 = wr.columns(AN, np.bincount(i.astype(np.int64), minlength=ANI), (sub, HOT_MAX))   # (sub 0: no lane)
    assert W == W0 if order in ("shuffled", "user") else W > 5 * W0, (order, W, W0)


@pytest.mark.parametrize("order", woc.ORDERS)
@pytest.mark.parametrize("sub", [0, 16])
def test_a_pair_windows_keep_the_documented_bounds(order, sub):
    u, p, q = woc.pairs(AN, ANU, ANI, SEED, order)
    t = _trainer(_pair_conf(ANU, ANI, 16), MB, [("window_pair_sub", sub)])
    ds = t.dataset_from_pairs(u, p, q)
    assert ds.kind == 8
    _bounds([p, q], ANI, ds.num_batches, sub, PAIR_MAX if sub else PER_MAX)   # both items of a pair count


@pytest.mark.parametrize("order", woc.ROW_ORDERS)
@pytest.mark.parametrize("ssub,isub", [(0, 0), (16, 0), (0, 32), (16, 32)])
def test_a_windows_of_rows_with_shared_user_ids_keep_the_documented_bounds(order, ssub, isub):
    ns = 150
    d, _, s, i = woc.shared_rows(AN, ANU, ns, ANI, SEED, order)
    conf = cases.conf_with(_conf(ANU + ns, ANI, 16), learning_rate="0.002")
    t = _trainer(conf, MB + [("amd:shared_user_from", ANU)], [("window_shared_sub", ssub), ("window_item_sub", isub)])
    ds = t.dataset_from_csr(d)
    W = ds.num_batches
    assert ds.kind == 8
    _bounds(i, ANI, W, isub, ITEM_MAX if isub else PER_MAX)
    _bounds(s, ns, W, ssub, SHARED_MAX if ssub else PER_MAX, PER_SHARED)


# ------------------------------------------------------------------------------------------------ b: the kernels on the windows of clustered files
def _oracle(conf, active=0, bf16=False):
    from oracle import oracle
    oracle.build()
    o = oracle.OracleTrainer("port", 0, active)
    if bf16:
        o.set_stale_rounding(True)
    o.seed(10)
    for k, v in conf:
        o.set_param(k, v)
    o.init_model()
    o.init_trainer()
    return o


def _check_windows(o, windows, passes, sub):
    """the checkers on a list of CSRData windows: update_window_substeps (sub > 0), else update_batch_stale plus the window's add"""
    for _ in range(passes):
        for d in windows:
            if sub > 0:
                o.update_window_substeps(d, sub)
            else:
                dW, db, _ = o.update_batch_stale(d)
                o.set_view("W_item", o.view("W_item") + dW)
                o.set_view("i_bias", o.view("i_bias") + db)
    return o


@pytest.fixture(scope="module")
def clustered_triples():
    return {order: woc.triples(AN, ANU, ANI, SEED + 1, order) for order in ("item", "burst")}


@pytest.mark.parametrize("order", ["item", "burst"])
@pytest.mark.parametrize("k", [10, 64, 128])
@pytest.mark.parametrize("mode", ["lane_off", "bf16", "lane_on"])
def test_b_triples_kernels_equal_the_checkers_on_clustered_windows(clustered_triples, order, k, mode):
    u, i, r = clustered_triples[order]
    conf = _conf(ANU, ANI, k)
    sub = HOT_SUB if mode == "lane_on" else 0
    t = _trainer(conf, MB + ([("amd:contrib", "bf16")] if mode == "bf16" else []), [("window_hot_sub", sub)])
    ds = t.dataset_from_triples(u, i, r)
    W = ds.num_batches
    assert ds.kind == 8 and W > 100, W                    # many small windows: a few dozen rows around one or two items on the item order
    for _ in range(2):
        t.train_dataset(ds)
    got = _views(t)
    wins = [sa.CSRData.from_triples(u[a:b], i[a:b], r[a:b]) for a, b in woc.window_cuts(AN, W)]
    o = _check_windows(_oracle(conf, bf16=mode == "bf16"), wins, 2, sub)
    for nm in NAMES:
        assert np.isfinite(got[nm]).all(), nm
        assert np.array_equal(got[nm].view(np.uint32), o.view(nm).view(np.uint32)), (nm, W)


@pytest.mark.parametrize("order", ["item", "burst"])
@pytest.mark.parametrize("k", [10, 64, 128])
def test_b_pair_kernels_equal_the_checker_on_clustered_windows(order, k):
    n, nu, ni = AN // 2, ANU // 2, ANI // 2               # (halved together: 800 slots per item, as above)
    u, p, q = woc.pairs(n, nu, ni, SEED + 2, order)
    conf = _pair_conf(nu, ni, k)
    t = _trainer(conf, MB)
    ds = t.dataset_from_pairs(u, p, q)
    W = ds.num_batches
    assert ds.kind == 8 and W > 100, W
    for _ in range(2):
        t.train_dataset(ds)
    got = _views(t, ("W_item", "i_bias", "W_user"))
    d = sa.pairs_as_csr(u, p, q)
    o = _check_windows(_oracle(conf, active=3), [d.slice_rows(a, b) for a, b in woc.window_cuts(n, W)], 2, 0)
    for nm in got:
        assert np.array_equal(got[nm].view(np.uint32), o.view(nm).view(np.uint32)), (nm, W)


@pytest.mark.parametrize("order", ["item", "burst"])
@pytest.mark.parametrize("k", [10, 64, 128])
def test_b_pair_lane_equals_the_checker_on_clustered_pairs(order, k):
    """window_pair_sub = 16: the sub-steps bound what is formed against one value of a row, so the windows stay large and a sorted item's slots
    are consecutive in the lane's file order (the pattern of tests/test_gpu_pair_hot_window.py, its small sizes: the checker is Python)"""
    n, nu, ni, s = 1600, 60, 40, 16
    u, p, q = woc.pairs(n, nu, ni, SEED + 3, order)
    conf = ph.conf(k, 3, 0, (("no_user_bias", "1"),), nu=nu, ni=ni)
    t = _trainer(conf, MB, [("window_pair_sub", s), ("window_pair_max", 64)])
    ds = t.dataset_from_pairs(u, p, q)
    W = ds.num_batches
    assert ds.kind == 8
    _bounds([p, q], ni, W, s, 64)
    assert ph.facts(p, q, W, s)["nhot"] >= 4
    for _ in range(2):
        t.train_dataset(ds)
    got = _views(t, ph.VIEWS)
    o = ph.check(conf, u, p, q, W, 2, s)
    _same(got, {nm: o.view(nm) for nm in ph.VIEWS}, (W,))


@pytest.mark.parametrize("order", ["item", "burst", "shared"])
@pytest.mark.parametrize("k,ssub,isub", [(10, 0, 0), (64, 0, 0), (128, 0, 0), (64, 4, 8)])
def test_b_rows_with_shared_user_ids_equal_the_checker_on_clustered_windows(order, k, ssub, isub):
    """the pattern of tests/test_gpu_shared_user_window.py at its small sizes (the checker is Python): 60 private users, 8 shared ids, 40 items"""
    n, npriv, ns, ni = 1600, 60, 8, 40
    d, _, s, i = woc.shared_rows(n, npriv, ns, ni, SEED + 4, order)
    conf = cases.conf_with(_conf(npriv + ns, ni, k), learning_rate="0.01")
    t = _trainer(conf, MB + [("amd:shared_user_from", npriv)], [("window_shared_sub", ssub), ("window_item_sub", isub), ("window_shared_max", 64), ("window_item_max", 64)])
    ds = t.dataset_from_csr(d)
    W = ds.num_batches
    assert ds.kind == 8
    _bounds(i, ni, W, isub, 64 if isub else PER_MAX)
    _bounds(s, ns, W, ssub, 64 if ssub else PER_MAX, PER_SHARED)
    for _ in range(2):
        t.train_dataset(ds)
    got = _views(t, ws.SHARED[:2] + ws.SHARED[3:])
    o = ws.make_oracle(conf)
    o = ws.simulate_rows(o, d, npriv, W, 2, isub=isub, sub=ssub)
    _same(got, {nm: o.view(nm) for nm in got}, (W,))


# ------------------------------------------------------------------------------------------------ c, d: accuracy
@pytest.fixture(scope="module")
def contract_inputs():
    """order -> (train, held out CSRData, held-out labels, the exact pass's held-out RMSE): the inputs of tests/test_window_orders.py"""
    out = {}
    for order in ("burst", "item"):
        train, held = woc.triples_with_holdout(N, NU, NI, SEED, order)
        test = sa.CSRData.from_triples(*held)
        t = _trainer(_conf(NU, NI, K))
        ds = t.dataset_from_triples(*train)
        assert ds.kind != 8
        out[order] = (train, test, held[2], _rmse_after(t, ds, test, held[2]))
    return out


def _rmse_after(t, ds, test, labels):
    for _ in range(3):
        t.train_dataset(ds)
    p = t.predict_batch(test)
    assert np.isfinite(p).all()
    return cases.rmse(p, labels)


@pytest.mark.parametrize("sub", [0, HOT_SUB])
def test_c_the_burst_order_keeps_the_accuracy_contract(contract_inputs, sub):
    train, test, labels, exact = contract_inputs["burst"]
    t = _trainer(_conf(NU, NI, K), MB, [("window_hot_sub", sub)])
    ds = t.dataset_from_triples(*train)
    assert ds.kind == 8
    got = _rmse_after(t, ds, test, labels)
    print("burst order, window_hot_sub", sub, "W", ds.num_batches, "dRMSE", got - exact)
    assert abs(got - exact) <= CONTRACT, (got, exact, ds.num_batches)


def test_d_auto_on_the_item_order(contract_inputs):
    """an item-sorted file is deep (every item is one chain), so `auto` weighs the window step without being asked: whichever it takes is sound"""
    train, test, labels, exact = contract_inputs["item"]
    t = _trainer(_conf(NU, NI, K), [("amd:step", "auto")])
    ds = t.dataset_from_triples(*train)
    if ds.kind == 8:
        m = _trainer(_conf(NU, NI, K), MB)
        assert ds.num_batches == m.dataset_from_triples(*train).num_batches
        _bounds(train[1], NI, ds.num_batches, HOT_SUB, HOT_MAX)
    got = _rmse_after(t, ds, test, labels)
    print("item order, auto: kind", ds.kind, "batches", ds.num_batches, "dRMSE", got - exact)
    assert abs(got - exact) <= (CONTRACT if ds.kind == 8 else 0.0), (ds.kind, got, exact)


# ------------------------------------------------------------------------------------------------ e: shuffled files are left alone
def _both_knobs(make, build, names):
    got = []
    for knob in (1, 0):
        t = make([("window_count_actual", knob)])
        ds = build(t)
        assert ds.kind == 8
        t.train_dataset(ds)
        got.append((ds.num_batches, _views(t, names)))
    assert got[0][0] == got[1][0] and got[0][0] > 1, (got[0][0], got[1][0])
    _same(got[0][1], got[1][1])


@pytest.mark.parametrize("seed,zipf", [(21, False), (22, False), (23, False), (21, True)])
@pytest.mark.parametrize("sub", [HOT_SUB, 0])
def test_e_shuffled_triples_keep_their_windows_and_bits(seed, zipf, sub):
    nu = 3000 if zipf else ANU
    u, i, r = woc.triples(AN, nu, ANI, seed, "shuffled", zipf=zipf)
    _both_knobs(lambda kn: _trainer(_conf(nu, ANI, 16), MB, [("window_hot_sub", sub)] + kn), lambda t: t.dataset_from_triples(u, i, r), NAMES)


@pytest.mark.parametrize("seed", [21, 22, 23])
@pytest.mark.parametrize("sub", [0, 16])
def test_e_shuffled_pairs_keep_their_windows_and_bits(seed, sub):
    u, p, q = woc.pairs(AN, ANU, ANI, seed, "shuffled")
    knobs = [("window_pair_sub", sub)] + ([("window_pair_max", 200)] if sub else [])   # (the cap low enough for more than one window)
    _both_knobs(lambda kn: _trainer(_pair_conf(ANU, ANI, 16), MB, knobs + kn), lambda t: t.dataset_from_pairs(u, p, q), ("W_item", "i_bias", "W_user"))


@pytest.mark.parametrize("seed", [21, 22, 23])
@pytest.mark.parametrize("ssub,isub", [(0, 0), (16, 32)])
def test_e_shuffled_rows_with_shared_user_ids_keep_their_windows_and_bits(seed, ssub, isub):
    ns = 150
    d = woc.shared_rows(AN, ANU, ns, ANI, seed, "shuffled")[0]
    conf = cases.conf_with(_conf(ANU + ns, ANI, 16), learning_rate="0.002")
    knobs = [("window_shared_sub", ssub), ("window_item_sub", isub)] + ([("window_shared_max", 200), ("window_item_max", 200)] if ssub else [])
    _both_knobs(lambda kn: _trainer(conf, MB + [("amd:shared_user_from", ANU)], knobs + kn), lambda t: t.dataset_from_csr(d), NAMES)


# ------------------------------------------------------------------------------------------------ f: knob 0 is the per-pass rule
@pytest.mark.parametrize("order", ["item", "burst"])
def test_f_knob_zero_is_the_per_pass_rule(order):
    (u, i, r), _ = woc.triples_with_holdout(N, NU, NI, SEED, order)
    for sub in (0, HOT_SUB):
        t = _trainer(_conf(NU, NI, K), MB, [("window_hot_sub", sub), ("window_count_actual", 0)])
        assert t.dataset_from_triples(u, i, r).num_batches == PARENT_W     # build only: this configuration is never trained
        t.set_knob("window_count_actual", 1)
        assert t.dataset_from_triples(u, i, r).num_batches == wr.as_cut(PARENT_W, [i], NI, sub, HOT_MAX if sub else PER_MAX)
    with pytest.raises(sa.SvdfError, match="window_count_actual must be 0 or 1"):
        t.set_knob("window_count_actual", 2)


def test_f_the_knob_is_part_of_the_schedule_signature():
    u, i, r = woc.triples(4000, 300, 50, SEED, "item")
    t = _trainer(_conf(300, 50, 16), MB)
    ds = t.dataset_from_triples(u, i, r)
    t.set_knob("window_count_actual", 0)
    with pytest.raises(sa.SvdfError, match="scheduled under another configuration"):
        t.train_dataset(ds)
    t.set_knob("window_count_actual", 1)
    t.train_dataset(ds)
    t.synchronize()


# ------------------------------------------------------------------------------------------------ g: window_hot_sub is recorded at build
def test_g_train_dataset_refuses_a_window_hot_sub_changed_since_the_build():
    u, i, r = woc.triples(6000, 300, 20, SEED, "shuffled")
    t = _trainer(_conf(300, 20, 16), MB, [("window_hot_sub", 16), ("window_hot_max", 160)])
    ds = t.dataset_from_triples(u, i, r)
    t.train_dataset(ds)
    for other in (8, 128, 0):
        t.set_knob("window_hot_sub", other)
        with pytest.raises(sa.SvdfError, match="built with another window_hot_sub"):
            t.train_dataset(ds)
    t.set_knob("window_hot_sub", 16)
    t.train_dataset(ds)
    t.synchronize()
    t.set_knob("window_hot_sub", 0)                      # a sequence built with the lane off is refused once it is on
    ds0 = t.dataset_from_triples(u, i, r)
    t.set_knob("window_hot_sub", 16)
    with pytest.raises(sa.SvdfError, match="built with another window_hot_sub"):
        t.train_dataset(ds0)

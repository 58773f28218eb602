"""Ordered sub-steps for hot ITEM rows on the csr path of the one-GPU window step (`amd:step = minibatch`, knobs `window_item_sub` /
`window_item_max`; svdf_wseq.cpp, svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_apply_hot<ITEM>).  An item-range row -- a plain item entry's
row, a feature_item child's row, or a row that is both -- with more than window_item_sub slots in a window is applied in file order, that many
slots at a time, every sub-step's changes formed against the row as the previous sub-step left it; everything else moves as in the plain window
step, hot shared user rows (section 6k) in their own lane.  Every view must equal the checker of tests/window_sim.py -- the pinned C port
driven one slot at a time -- bit for bit.  With the knob at 0 (the default) nothing changes."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import CSRData

pytestmark = pytest.mark.gpu

NP = 60                     # private users
NT, NA, NG = 40, 30, 6      # tracks, item attribute ids after them (feature_item children), global ids
NI = NT + NA
HOT_TRACKS = (0, 1, 2)      # drawn with p = 0.8
A_HOT, A_BOTH, A_COLD_PARENTS = NT, NT + 1, NT + 2
VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")
IVALS = (1.0, 0.5, -0.75, 1.25)


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


def _conf(k, ns, reg=0, extra=(), active=0):
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NP + ns, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01", active_type=active) + list(extra)
    return cases.conf_with(conf, base_score="0.5") if active != 0 else conf


def _assert_same(t, o):
    for name in VIEWS:
        a, b = t.view(name), o.view(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def _table(rng):
    """attribute ids behind the tracks: A_HOT behind the hot tracks 0 and 1 (a hot child whose parent is hot too), A_BOTH behind track 1 and a
    plain entry of other rows (hot both ways), nothing behind hot track 2, A_COLD_PARENTS behind every other track (a hot child whose parents
    are cold), and rare attributes here and there (cold children)"""
    rows = []
    for tr in range(NT):
        if tr == 0:
            ch = [A_HOT, NT + 5]
        elif tr == 1:
            ch = [A_HOT, A_BOTH]
        elif tr == 2:
            ch = []
        else:
            ch = [A_COLD_PARENTS] + ([int(rng.integers(NT + 6, NI))] if rng.random() < 0.5 else [])
        rows.append([(c, float(rng.choice([1.0, 0.5, 0.25, 2.0, 0.75]))) for c in ch])
    return rows


def _rows(rng, n, ns=0, ivals=True, second=0.35, both=0.3, hot_users=(), logistic=False):
    """(0 .. 2 globals, the private user [+ shared user ids], 1 .. 3 items): the first item is a hot track with p = 0.8; a second item with
    p = `second`, a hot track half of the time (two hot items in one data row); A_BOTH as a plain entry with p = `both`"""
    rows = []
    for _ in range(n):
        g = sorted(int(x) for x in rng.choice(NG, size=int(rng.integers(0, 3)), replace=False))
        users = [(int(rng.integers(0, NP)), float(rng.choice([1.0, 0.5, 1.5])))]
        if ns:
            sh = []
            if hot_users and rng.random() < 0.8:
                sh.append(int(rng.choice(hot_users)))
            for _ in range(int(rng.integers(0, 2))):
                x = NP + int(rng.integers(0, ns))
                if x not in sh:
                    sh.append(x)
            sh = [(s, float(rng.choice([1.0, 0.5, 2.0]))) for s in sh]
            at = int(rng.integers(0, len(sh) + 1))
            users = sh[:at] + users + sh[at:]
        it = [int(rng.choice(HOT_TRACKS)) if rng.random() < 0.8 else int(rng.integers(3, NT))]
        if rng.random() < second:
            x = int(rng.choice(HOT_TRACKS)) if rng.random() < 0.5 else int(rng.integers(3, NT))
            if x not in it:
                it.append(x)
        if rng.random() < both:
            it.insert(int(rng.integers(0, len(it) + 1)), A_BOTH)
        items = [(x, float(rng.choice(IVALS)) if ivals else 1.0) for x in it]
        label = float(rng.random() < 0.5) if logistic else float(rng.integers(1, 6))
        rows.append((label, [(x, float(rng.uniform(0.1, 1.0))) for x in g], users, items))
    return CSRData.from_rows(rows)


def _facts(d, B, window, isub, sub, fu, fi):
    """what the data holds, window by window: hot item rows, hot user rows, a ragged last sub-step, and the shapes the lane must cover"""
    f = dict(nhot=0, nuhot=0, ragged=False, plain=False, child_cold_parent=False, child_hot_parent=False, both=False, two_in_row=False,
             user_and_item=False, most=0)
    for b0 in range(0, d.num_row, window):
        win = d.slice_rows(b0, min(b0 + window, d.num_row))
        ic = ws.item_slot_counts(win, B, fu, fi)
        uc = {}
        for r in range(win.num_row):
            _, ng, nu, _, idx, _ = win.row(r)
            for u in ws.row_targets(idx, ng, nu, B, fu, fi)[0]:
                uc[u] = uc.get(u, 0) + 1
        ihot = {i for i, c in ic.items() if c > isub}
        uhot = {u for u, c in uc.items() if c > sub} if sub > 0 else set()
        f["nhot"] += len(ihot)
        f["nuhot"] += len(uhot)
        f["ragged"] = f["ragged"] or any(ic[i] % isub for i in ihot)
        f["most"] = max([f["most"]] + [ic[i] for i in ihot])
        as_entry, as_child = set(), set()
        for r in range(win.num_row):
            _, ng, nu, _, idx, _ = win.row(r)
            entries = [int(x) for x in idx[ng + nu:]]
            users, items = ws.row_targets(idx, ng, nu, B, fu, fi)
            as_entry |= set(entries) & ihot
            for p in entries:
                for c in ws.children(fi, [p]):
                    if c in ihot:
                        as_child.add(c)
                        f["child_hot_parent" if p in ihot else "child_cold_parent"] = True
            f["two_in_row"] = f["two_in_row"] or sum(i in ihot for i in items) >= 2
            f["user_and_item"] = f["user_and_item"] or (any(u in uhot for u in users) and any(i in ihot for i in items))
        f["plain"] = f["plain"] or bool(as_entry - as_child)
        f["both"] = f["both"] or bool(as_entry & as_child)
    return f


def _ip():
    return (("ip:wd", "0.01"), ("ip:bound", "2"), ("ip:wd", "0.003"), ("ip:bound", str(NT + 1)), ("ip:wd", "0.02"), ("ip:bound", str(NI)))


def _run(tmp_path, k, active, reg, extra, isub, ns=0, sub=0, table="item", window=90, n=330, passes=2, seed=None, plain_differs="W_item"):
    """one case: the data, what it must hold, two passes on the GPU against the checker; returns (facts, data, trainer views)"""
    extra = _ip() if extra == "ip" else extra
    rng = np.random.default_rng(1000 + k + reg + isub if seed is None else seed)
    keys, tu, ti = [], [], []
    if table in ("item", "both"):
        ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), _table(rng)))
        keys.append(("feature_item", str(tmp_path / "fi.txt")))
    if table == "both":
        tu = ws.read_table(ws.write_table(str(tmp_path / "fu.txt"), ws.random_table(rng, NP + ns, NP, NP + ns, 2, hot=(NP, NP + 1), hot_p=0.7)))
        keys.append(("feature_user", str(tmp_path / "fu.txt")))
    conf = _conf(k, ns, reg, extra, active) + keys
    B = NP   # with ns = 0 there is no id >= B: no shared user row, and the trainer never hears of amd:shared_user_from
    d = _rows(rng, n, ns, hot_users=(NP, NP + 1, NP + 2) if ns else (), logistic=active != 0)
    d = ws.drop_rows_reaching_twice(d, B, tu, ti)
    f = _facts(d, B, window, isub, sub, tu, ti)
    params = [("amd:step", "minibatch"), ("amd:window", window)] + ([("amd:shared_user_from", NP)] if ns else [])
    knobs = [("window_item_sub", isub)] + ([("window_shared_sub", sub)] if sub else [])
    t = _trainer(conf, active, params, knobs)
    ds = t.dataset_from_csr(d)
    W = ds.num_batches
    assert ds.kind == 8 and W == (d.num_row + window - 1) // window   # with amd:window the window size is the caller's
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    ub = dict(extra).get("no_user_bias") != "1"
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, B, W, passes, isub=isub, sub=sub, fu=tu, fi=ti, user_bias=ub)
    _assert_same(t, o)
    # the lane did something: the plain window step ends elsewhere
    p = ws.simulate_rows(ws.make_oracle(conf, active=active), d, B, W, passes, fu=tu, fi=ti, user_bias=ub)
    assert not np.array_equal(p.view(plain_differs)[0], o.view(plain_differs)[0])
    return f, d, t


# (k, active_type, reg_method, extra keys, window_item_sub): feature_item loaded, no amd:shared_user_from -- rows of globals + one user + items
ITEMS = [
    (1, 0, 0, (), 1),
    (3, 0, 1, (("wd_item_bias", "0.01"),), 3),
    (7, 2, 3, (), 5),
    (16, 3, 2, "ip", 12),
    (64, 0, 0, "ip", 12),
    (64, 0, 1, (("no_user_bias", "1"), ("wd_item_bias", "0.02")), 5),
    (64, 2, 2, (), 3),
    (100, 0, 3, "ip", 1),
    (128, 3, 0, (("no_user_bias", "1"), ("wd_item_bias", "0.01")), 1),
    (200, 0, 2, (("user_nonnegative", "1"),), 12),
    (256, 0, 1, "ip", 5),
    (256, 2, 0, (("wd_user_bias", "0.005"), ("wd_item_bias", "0.01")), 3),
]


@pytest.mark.parametrize("k,active,reg,extra,isub", ITEMS)
def test_hot_item_rows_in_sub_steps_equal_the_checker(tmp_path, k, active, reg, extra, isub):
    f, d, _ = _run(tmp_path, k, active, reg, extra, isub)
    assert d.num_row > 250 and f["nhot"] >= 8 and (f["ragged"] or isub == 1)
    # a hot plain item, a hot child behind cold parents, a hot child behind a hot parent, a row hot both as an entry and as a child, and two
    # hot rows met by one data row
    assert f["plain"] and f["child_cold_parent"] and f["child_hot_parent"] and f["both"] and f["two_in_row"]
    assert np.any(d.feat_value[d.row_ptr[2:-1:3]] != 1.0)   # item values other than 1


def test_plain_items_without_a_table_or_shared_users(tmp_path):
    """no side table and no amd:shared_user_from: globals + one user + items through wseq_from_csr, hot plain items only"""
    f, d, _ = _run(tmp_path, 64, 0, 0, (("wd_item_bias", "0.01"),), 5, table="none")
    assert f["nhot"] >= 8 and f["ragged"] and f["plain"] and f["two_in_row"] and not f["child_hot_parent"] and not f["child_cold_parent"]


def test_one_window_with_sub_steps_of_128_spans_lane_group_rounds(tmp_path):
    """window_item_sub = 128 on a single 330-row window at k = 64 (16 lanes per slot, 16 lane groups): the hottest row's first sub-step is 8 full
    lane-group rounds, its last sub-step ends on a partial one"""
    f, d, _ = _run(tmp_path, 64, 0, 0, (("wd_item_bias", "0.01"),), 128, window=330, seed=77)
    assert d.num_row <= 330 and f["nhot"] >= 1 and f["most"] > 128 + 16 and (f["most"] - 128) % 16 != 0


# (k, active_type, reg_method, extra keys, window_item_sub, window_shared_sub, tables): amd:shared_user_from with three hot shared ids
SHARED = [
    (5, 0, 0, (), 3, 0, "item"),
    (16, 2, 3, "ip", 5, 3, "item"),
    (64, 0, 0, (("wd_item_bias", "0.01"),), 12, 12, "both"),
    (64, 3, 1, (("no_user_bias", "1"),), 3, 5, "both"),
    (128, 0, 2, "ip", 1, 1, "none"),
    (256, 0, 3, (("user_nonnegative", "1"), ("wd_user_bias", "0.005")), 5, 12, "both"),
]


@pytest.mark.parametrize("k,active,reg,extra,isub,sub,table", SHARED)
def test_hot_item_rows_next_to_shared_user_rows(tmp_path, k, active, reg, extra, isub, sub, table):
    # (a feature_user table makes half of the rows reach a shared user row twice, and those are dropped: draw twice as many)
    f, d, _ = _run(tmp_path, k, active, reg, extra, isub, ns=40, sub=sub, table=table, n=660 if table == "both" else 330)
    assert d.num_row > 150 and f["nhot"] >= 8 and f["two_in_row"]
    if sub:   # both lanes in one window, and a data row that holds a hot user entry and a hot item entry
        assert f["nuhot"] >= 4 and f["user_and_item"]


def _zero_case(tmp_path):
    rng = np.random.default_rng(5)
    ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), _table(rng)))
    conf = _conf(32, 0) + [("feature_item", str(tmp_path / "fi.txt"))]
    return conf, ws.drop_rows_reaching_twice(_rows(rng, 2000), NP, [], ti)


def test_knob_at_zero_is_the_knob_unset(tmp_path):
    """the default rule, the same windows and the same bits; and the lane, once switched on (sub-steps of 3, the children's class value: the
    cap alone sets the item side's windows), is what moves the result"""
    conf, d = _zero_case(tmp_path)
    got = []
    for knobs in ((), (("window_item_sub", 0),), (("window_item_sub", 0), ("window_item_max", 32)), (("window_item_sub", 3),)):
        t = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=knobs)
        ds = t.dataset_from_csr(d)
        for _ in range(2):
            t.train_dataset(ds)
        t.synchronize()
        got.append((ds.kind, ds.num_batches, {name: t.view(name).copy() for name in VIEWS}))
    assert got[0][:2] == got[1][:2] == got[2][:2] and got[0][0] == 8
    for other in got[1:3]:
        for name in VIEWS:
            assert np.array_equal(got[0][2][name].view(np.uint32), other[2][name].view(np.uint32)), name
    assert got[3][1] < got[0][1] and not np.array_equal(got[0][2]["W_item"][:3], got[3][2]["W_item"][:3])


def test_window_rule_with_sub_steps(tmp_path):
    conf, d = _zero_case(tmp_path)
    ti = ws.read_table(str(tmp_path / "fi.txt"))
    counts = ws.item_slot_counts(d, NP, (), ti)
    ci, child = np.zeros(NI, np.int64), np.zeros(NI, np.uint8)   # the pass's slots of every item-range row; the rows that are a feature_item child
    for i, n in counts.items():
        ci[i] = n
    for row in ti:
        for c, _ in row:
            child[c] = 1
    globs = np.bincount(np.concatenate([d.row(r)[4][:d.row(r)[1]] for r in range(d.num_row)]).astype(np.int64), minlength=NG)
    t = _trainer(conf, extra=[("amd:step", "minibatch")])
    default = t.dataset_from_csr(d).num_batches
    assert default == wr.csr(d.num_row, ci, globs, item_child=child)
    for sub, cap in ((3, 2048), (3, 64), (2, 256), (8, 128), (24, 512)):
        t.set_knob("window_item_sub", sub)
        t.set_knob("window_item_max", cap)
        W = t.dataset_from_csr(d).num_batches
        assert W == wr.csr(d.num_row, ci, globs, item_child=child, item_lane=(sub, cap)), (sub, cap)
        assert W <= default
    t.set_knob("window_item_sub", 3)
    t.set_knob("window_item_max", 2048)
    assert t.dataset_from_csr(d).num_batches < default


def test_train_dataset_refuses_a_knob_changed_since_the_build(tmp_path):
    conf, d = _zero_case(tmp_path)
    t = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=[("window_item_sub", 8)])
    ds = t.dataset_from_csr(d)
    t.train_dataset(ds)
    for other in (3, 0):
        t.set_knob("window_item_sub", other)
        with pytest.raises(sa.SvdfError, match="built with another window_item_sub"):
            t.train_dataset(ds)
    t.set_knob("window_item_sub", 8)
    t.train_dataset(ds)
    t.synchronize()
    with pytest.raises(sa.SvdfError, match=r"window_item_sub must be in 0 \.\. 128"):
        t.set_knob("window_item_sub", 129)
    with pytest.raises(sa.SvdfError, match=r"window_item_sub must be in 0 \.\. 128"):
        t.set_knob("window_item_sub", -1)
    with pytest.raises(sa.SvdfError, match="window_item_max must be positive"):
        t.set_knob("window_item_max", 0)


def test_refusals_name_their_cause():
    one = CSRData.from_rows([(3.0, [(1, 0.5)], [(0, 1.0)], [(2, 1.0)])])
    mb = [("amd:step", "minibatch")]
    # bf16 contribution rows
    t = _trainer(_conf(8, 0), 0, mb + [("amd:contrib", "bf16")], [("window_item_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"window_item_sub > 0 \(ordered sub-steps for hot item rows\) needs amd:contrib = fp32"):
        t.dataset_from_csr(one)
    # every contribution through a slot
    t = _trainer(_conf(8, 0), 0, mb, [("window_item_sub", 12), ("wunit_inplace", 0)])
    with pytest.raises(sa.SvdfError, match=r"window_item_sub > 0 .* needs the in-place sums \(knob wunit_inplace = 1\)"):
        t.dataset_from_csr(one)
    # the N-rank window builder
    t = _trainer(_conf(8, 0), 0, [], [("window_item_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"svdf_dataset_window_from_csr: window_item_sub > 0 .* is for the one-GPU window sequence"):
        t.dataset_window_from_csr(one)
    # user-group (SVD++) trainers
    blocks = cases.user_blocks(6, 20, NT, NT, seed=2)
    g = sa.Trainer(1, 0)
    g.seed(10)
    for k_, v_ in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=NI, num_factor=8, num_ufeedback=NT) + mb:
        g.set_param(k_, str(v_))
    g.init_model()
    g.init_trainer()
    g.set_knob("window_item_sub", 12)
    with pytest.raises(sa.SvdfError, match=r"window_item_sub > 0 .* is not supported with user-group \(SVD\+\+\) trainers"):
        g.dataset_from_blocks(blocks)
    g.set_knob("window_item_sub", 0)
    g.dataset_from_blocks(blocks).close()


@pytest.mark.parametrize("isub,sub,batch", [(8, 0, 500), (8, 5, 0)])
def test_the_staged_route_honours_the_knob(tmp_path, isub, sub, batch):
    """update_csr_batch / update_csr under amd:step = minibatch with the knob == the resident route, chunk by chunk (the pattern of
    tests/test_gpu_staged_window.py), and != the same feed with the knob at 0"""
    from test_gpu_staged_window import _cuts, _feed, _resident, _same, _views, _differ
    rng = np.random.default_rng(11)
    ns, S = 40, 1024
    ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), _table(rng)))
    conf = _conf(32, ns) + [("feature_item", str(tmp_path / "fi.txt"))]
    d = ws.drop_rows_reaching_twice(_rows(rng, 2600, ns, hot_users=(NP, NP + 1, NP + 2)), NP, [], ti)
    params = [("amd:step", "minibatch"), ("amd:window", 256), ("amd:shared_user_from", NP)]
    make = lambda i, s: _trainer(conf, extra=params, knobs=[("stage_window", S), ("window_item_sub", i), ("window_shared_sub", s)])   # noqa: E731
    cuts = _cuts(d.num_row, batch, S)
    assert len(cuts) >= 2
    assert max(ws.item_slot_counts(d.slice_rows(0, 256), NP, (), ti).values()) > isub
    t = make(isub, sub)
    _feed(t, d, batch)
    r = _resident(make(isub, sub), d, cuts, lambda t_, a, b: t_.dataset_from_csr(d.slice_rows(a, b)))
    z = make(0, sub)
    _feed(z, d, batch)
    got = _views(t)
    assert all(np.isfinite(v).all() for v in got.values())
    _same(got, _views(r))
    assert _differ(got, _views(z))
    assert t.counter(30) == len(cuts) and t.counter(31) == 0


def test_staged_chunks_without_the_in_place_sums_keep_the_exact_step(tmp_path, capfd):
    """window_item_sub > 0 with knob wunit_inplace = 0: decided before the build -- the chunks train exactly, nothing raises"""
    from test_gpu_staged_window import _cuts, _feed, _same, _views
    conf, d = _zero_case(tmp_path)
    knobs = [("stage_window", 1024), ("window_item_sub", 8), ("wunit_inplace", 0)]
    t = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=knobs)
    e = _trainer(conf, knobs=knobs)
    _feed(t, d, 500)
    _feed(e, d, 500)
    _same(_views(t), _views(e))
    assert t.counter(30) == 0 and t.counter(31) == len(_cuts(d.num_row, 500, 1024))
    assert "window_item_sub" in capfd.readouterr().err


def test_short_fuzz_run():
    import fuzz_item_hot
    assert fuzz_item_hot.run(iters=12, seed=7) == 0

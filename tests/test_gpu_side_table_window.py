"""feature_user / feature_item side tables in the one-GPU window step (`amd:step = minibatch`; svdf_wunit.cpp, svdf_k_wunit.hip; DESIGN.md
section 6j).  Every child is a shared target: read as of the window start, its change summed per row in file order at the window's end (or
applied in place when it is the row's only contribution).  feature_user children are shared user rows (ids >= amd:shared_user_from);
feature_item children keep the reference's item-side forms (apex_svd_base.h:313-427).  Every view must equal the checker of
tests/window_sim.py -- the pinned C port loading the same table files, row by row on the window-start shared rows -- bit for bit."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import CSRData

pytestmark = pytest.mark.gpu

NP, NS = 60, 100            # private users, shared user ids (B = NP)
NT, NA, NG = 40, 30, 6      # tracks, item attribute ids after them (album / artist / genre rows), global ids
NI = NT + NA
HOT_U = (NP, NP + 1)        # hot feature_user children: many slots per window; the other children are mostly applied in place
HOT_I = (NT, NT + 1)        # hot feature_item children
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


def _tables(tmp_path, seed, which):
    """(conf keys, user table, item table): user children of every user id drawn from the shared ids, item children of every track drawn
    from the attribute ids (the attribute ids themselves have no table row)"""
    rng = np.random.default_rng(seed)
    keys, tu, ti = [], [], []
    if which in ("user", "both"):
        tu = ws.read_table(ws.write_table(str(tmp_path / "fu.txt"), ws.random_table(rng, NP + NS, NP, NP + NS, 2, hot=HOT_U, hot_p=0.7)))
        keys.append(("feature_user", str(tmp_path / "fu.txt")))
    if which in ("item", "both"):
        ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), ws.random_table(rng, NT, NT, NI, 3, hot=HOT_I, hot_p=0.7)))
        keys.append(("feature_item", str(tmp_path / "fi.txt")))
    return keys, tu, ti


def _data(seed, tu, ti, n=360, positions=("first", "middle", "last"), max_shared=2, binary=False):
    rng = np.random.default_rng(seed)
    d = ws.table_rows(rng, n, NP, NS, NT, num_global=NG, max_g=2, max_shared=max_shared, max_items=2, uvals=True, ivals=True,
                       positions=positions)
    d = ws.drop_rows_reaching_twice(d, NP, tu, ti)
    if binary:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    return d


def _assert_same(t, o):
    for name in VIEWS:
        a, b = t.view(name), o.view(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


UP = (("up:wd", "0.01"), ("up:bound", "90"), ("up:wd", "0.003"), ("up:bound", str(NP + NS)))
IP = (("ip:wd", "0.002"), ("ip:bound", str(NT + 5)), ("ip:wd", "0.02"), ("ip:bound", str(NI)))
CASES = [  # (k, active_type, reg_method, extra keys, private positions, tables, amd:shared_user_from)
    (1, 0, 0, (), ("first",), "user", True),
    (7, 0, 1, (("user_nonnegative", "1"),), ("first",), "item", False),
    (16, 2, 3, (), ("last",), "both", True),
    (64, 0, 0, (), ("first", "middle", "last"), "both", True),
    (64, 3, 1, (("no_user_bias", "1"),), ("first", "middle", "last"), "both", True),
    (128, 0, 2, UP + IP, ("first", "middle", "last"), "both", True),
    (128, 2, 0, (("no_user_bias", "1"), ("wd_user_bias", "0.01"), ("wd_item_bias", "0.02")), ("middle", "last"), "item", True),
    (256, 0, 3, UP + (("wd_item_bias", "0.01"), ("wd_user_bias", "0.005")), ("first", "last"), "user", True),
    (256, 3, 2, IP, ("first", "middle", "last"), "both", True),
]


@pytest.mark.parametrize("k,active,reg,extra,positions,which,key", CASES)
def test_minibatch_with_side_tables_equals_the_checker(tmp_path, k, active, reg, extra, positions, which, key):
    keys, tu, ti = _tables(tmp_path, k + reg, which)
    conf = cases.conf_with(_conf(k, reg, extra), active_type=active) + keys
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    d = _data(k + reg, tu, ti, positions=positions, max_shared=2 if key else 0, binary=active != 0)
    B = NP if key else NP + NS
    nkids = sum(len(ws.children(tu, [int(x) for x in d.row(r)[4][d.row(r)[1]:d.row(r)[1] + d.row(r)[2]]])) +
                len(ws.children(ti, [int(x) for x in d.row(r)[4][d.row(r)[1] + d.row(r)[2]:]])) for r in range(d.num_row))
    assert d.num_row > 200 and nkids > 150
    t = _trainer(conf, active, [("amd:step", "minibatch"), ("amd:window", 90)] + ([("amd:shared_user_from", NP)] if key else []))
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8
    W = ds.num_batches
    assert W == (d.num_row + 89) // 90
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, B, W, 2, fu=tu, fi=ti, user_bias=dict(extra).get("no_user_bias") != "1")
    _assert_same(t, o)


def test_a_table_that_covers_none_of_the_data_changes_nothing(tmp_path):
    """children only for ids the data never uses: the same windows and bits as without the tables"""
    rng = np.random.default_rng(4)
    tu = [[] for _ in range(NP)] + ws.random_table(rng, NS, NP, NP + NS, 2)          # only shared ids >= NP have children: rows use none
    ti = [[] for _ in range(NT // 2)] + ws.random_table(rng, NT // 2, NT, NI, 3)    # only tracks >= NT / 2 have children
    fu, fi = ws.write_table(str(tmp_path / "fu.txt"), tu), ws.write_table(str(tmp_path / "fi.txt"), ti)
    r2 = np.random.default_rng(5)
    d = ws.table_rows(r2, 300, NP, NS, NT // 2, num_global=NG, max_g=2, max_shared=0, max_items=2, uvals=True, ivals=True)
    got = []
    for keys in ([], [("feature_user", fu), ("feature_item", fi)]):
        t = _trainer(_conf(64) + keys, 0, [("amd:step", "minibatch"), ("amd:window", 70), ("amd:shared_user_from", NP)])
        ds = t.dataset_from_csr(d)
        for _ in range(2):
            t.train_dataset(ds)
        t.synchronize()
        got.append((ds.kind, ds.num_batches, {name: t.view(name).copy() for name in VIEWS}))
    assert got[0][:2] == got[1][:2] == (8, 5)
    for name in VIEWS:
        assert np.array_equal(got[0][2][name].view(np.uint32), got[1][2][name].view(np.uint32)), name


def _deep(tmp_path, n=20000, seed=3):
    """300 users, 200 tracks; every user a child among 4 buckets (ids 300 ..), every track a child among 4 genres (ids 200 ..): the exact
    levels are n / 4 deep"""
    fu = ws.write_table(str(tmp_path / "fu.txt"), [[(300 + u % 4, 1.0)] for u in range(300)])
    fi = ws.write_table(str(tmp_path / "fi.txt"), [[(200 + i % 4, 0.5)] for i in range(200)])
    rng = np.random.default_rng(seed)
    rows = [(float(rng.integers(1, 6)), [(int(rng.integers(0, 8)), float(rng.uniform(0.1, 1.0)))], [(int(rng.integers(0, 300)), 1.0)],
             [(int(rng.integers(0, 200)), 1.0)]) for _ in range(n)]
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=204, num_global=8, num_factor=32, wd_global="0.001")
    return conf + [("feature_user", fu), ("feature_item", fi)], CSRData.from_rows(rows)


def test_auto_keeps_the_exact_pass_with_a_table_loaded(tmp_path):
    conf, d = _deep(tmp_path)
    t = _trainer(conf, extra=[("amd:step", "auto"), ("amd:shared_user_from", 300)])
    ds = t.dataset_from_csr(d)
    assert t.counter(16) == 3 and ds.kind != 8
    e = _trainer(conf)
    de = e.dataset_from_csr(d)
    assert de.kind == ds.kind and de.num_batches == ds.num_batches
    for _ in range(2):
        t.train_dataset(ds)
        e.train_dataset(de)
    t.synchronize(); e.synchronize()
    _assert_same(t, e)


def test_default_window_rule_counts_children_at_3_updates_per_window(tmp_path):
    """the 4 bucket rows and the 4 genre rows are met by n / 4 rows each: as child targets they set the window count at
    window_per_target_child (3) updates per window on average -- not at the 12 of shared user rows or the 24 of item rows, which miss the
    accuracy contract on the variant of tools/sidetable_window.py"""
    conf, d = _deep(tmp_path)
    uid = d.feat_index[d.row_ptr[1:-1:3]].astype(np.int64)
    iid = d.feat_index[d.row_ptr[2:-1:3]].astype(np.int64)
    counts = np.concatenate([np.bincount(uid % 4, minlength=4), np.bincount(iid % 4, minlength=4)]).astype(np.float64)
    met = wr.met(counts, 0.0)   # sum c^2 / sum c over the child targets (the most updates of one row do not bind here)
    t = _trainer(conf, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)])
    assert t.dataset_from_csr(d).num_batches == int(np.ceil(met / 3))
    t.set_knob("window_per_target_shared", 1)   # the shared user rows' knob does not move child rows
    assert t.dataset_from_csr(d).num_batches == int(np.ceil(met / 3))
    t.set_knob("window_per_target_child", 12)
    assert t.dataset_from_csr(d).num_batches == int(np.ceil(met / 12))


def test_refusals_name_their_cause(tmp_path):
    fu = ws.write_table(str(tmp_path / "fu.txt"), [[(NP + 5, 1.0)], [(NP + 6, 0.5), (NP + 7, 1.0)]])
    low = ws.write_table(str(tmp_path / "low.txt"), [[(NP + 5, 1.0)], [(3, 1.0)]])
    fi = ws.write_table(str(tmp_path / "fi.txt"), [[(NT + 1, 1.0)], [(NT + 1, 0.5)], [(NT + 2, 1.0)]])
    mb = [("amd:step", "minibatch"), ("amd:shared_user_from", NP)]
    one = CSRData.from_rows([(3.0, [], [(0, 1.0)], [(2, 1.0)])])
    # a feature_user table without amd:shared_user_from
    t = _trainer(_conf(8) + [("feature_user", fu)], 0, [("amd:step", "minibatch")])
    with pytest.raises(sa.SvdfError, match="feature_user side table needs amd:shared_user_from"):
        t.dataset_from_csr(one)
    # a user child below B
    t = _trainer(_conf(8) + [("feature_user", low)], 0, mb)
    with pytest.raises(sa.SvdfError, match="feature_user child below amd:shared_user_from"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(1, 1.0)], [(2, 1.0)])]))
    t.dataset_from_csr(one).close()   # user 0's child is a shared row
    # one target twice after the expansion
    t = _trainer(_conf(8) + [("feature_user", fu), ("feature_item", fi)], 0, mb)
    with pytest.raises(sa.SvdfError, match="reaches one item row twice through feature_item children"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(0, 1.0)], [(0, 1.0), (1, 1.0)])]))   # two tracks of one album
    with pytest.raises(sa.SvdfError, match="reaches one item row twice through feature_item children"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(0, 1.0)], [(2, 1.0), (NT + 2, 1.0)])]))   # a track listed with its own album
    with pytest.raises(sa.SvdfError, match="reaches one user row twice through feature_user children"):
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(1, 1.0), (NP + 7, 1.0)], [(2, 1.0)])]))
    with pytest.raises(sa.SvdfError, match="an item id listed twice in one row"):   # a plain repeat keeps the builder's own message
        t.dataset_from_csr(CSRData.from_rows([(3.0, [], [(5, 1.0)], [(9, 1.0), (9, 1.0)])]))
    # bf16 contribution rows
    t = _trainer(_conf(8) + [("feature_item", fi)], 0, [("amd:step", "minibatch"), ("amd:contrib", "bf16")])
    with pytest.raises(sa.SvdfError, match="side tables need amd:contrib = fp32"):
        t.dataset_from_csr(one)
    # the N-rank window builder
    t = _trainer(_conf(8) + [("feature_item", fi)], 0)
    with pytest.raises(sa.SvdfError, match="svdf_dataset_window_from_csr: feature_user / feature_item side tables"):
        t.dataset_window_from_csr(one)
    # user-group (SVD++) trainers
    blocks = cases.user_blocks(6, 20, NT, NT, seed=2)
    g = sa.Trainer(1, 0)
    g.seed(10)
    for k_, v_ in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=NI, num_factor=8, num_ufeedback=NT) + [("feature_item", fi),
                                                                                                                   ("amd:step", "minibatch")]:
        g.set_param(k_, str(v_))
    g.init_model()
    g.init_trainer()
    with pytest.raises(sa.SvdfError, match="user-group \\(SVD\\+\\+\\) trainers"):
        g.dataset_from_blocks(blocks)


def test_short_fuzz_run():
    import fuzz_side_table
    assert fuzz_side_table.run(iters=10, seed=7) == 0

"""Ordered sub-steps for hot shared user rows of user-group (SVD++) blocks in the one-GPU window step (knobs `window_block_sub`, `window_block_max`
under `amd:shared_user_from = B` on a format_type 1 trainer; svdf_wseq.cpp, svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_walk<LPI, true, true> and
k_wunit_apply_hot<LPI, false, true>).  A shared user row with more than `window_block_sub` slots in a window is applied in
file order, that many slots at a time, every slot computed from the span state the walk held when it reached the data row (private row and bias,
tmp_ufeedback and its bias).  All seven views must equal the checker of tests/window_sim.py -- the pinned C port of SVDPPFeature::update with
every hot slot's span replayed from its start -- bit for bit, and counter 35 the checker's count of hot rows."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

pytestmark = pytest.mark.gpu

NP, NS, NI, NF = 60, 8, 40, 40      # private users, shared user ids (B = NP), items, feedback ids: the shape of tests/test_gpu_block_shared_window.py
VIEWS = ws.VIEWS
SVDPP = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
MB = [("amd:step", "minibatch"), ("amd:shared_user_from", NP)]
SPLIT = (("up:wd", "0.01"), ("up:bound", str(NP + 3)), ("up:wd", "0.003"), ("up:bound", str(NP + NS)))   # wd_user ranges that split the shared ids


@pytest.fixture(scope="module", autouse=True)
def _port():
    from oracle import oracle
    oracle.build()


def _trainer(conf, active=0, extra=(), knobs=()):
    t = sa.Trainer(1, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _conf(k, active=0, reg=0, extra=(), nf=NF, ng=0):
    c = cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_global=ng, num_factor=k, num_ufeedback=nf, reg_method=reg,
                        active_type=active, learning_rate="0.01", wd_global="0.002") + SVDPP + list(extra)
    return cases.conf_with(c, base_score="0.5") if active else c


def _blocks(seed, n=75, **kw):
    return ws.shared_blocks(np.random.default_rng(seed), n, NP, NS, NI, kw.pop("num_fb", NF), **kw)


def _window_key(ba, windows=3):
    return [("amd:window", -(-ba.num_row // windows))]


def _views(t):
    return {name: (t.view(name).copy() if t.view(name) is not None else None) for name in VIEWS}


def _same(a, b):
    for name in VIEWS:
        x, y = a[name], b[name]
        if x is None or y is None or x.size == 0:
            continue
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), name


def _run(conf, ba, active=0, knobs=(), passes=2, extra=MB, sub=0):
    t = _trainer(conf, active, list(extra) + _window_key(ba), list(knobs) + ([("window_block_sub", sub)] if sub is not None else []))
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches == 3, (ds.kind, ds.num_batches)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    return t, ds


def _against_checker(conf, ba, sub, active=0, knobs=(), user_bias=True, hot=True, passes=2):
    """2 passes of 3 windows against window_sim.step_blocks; counter 35 = the checker's hot rows (hot: some / none), the windows under counter 34"""
    t, ds = _run(conf, ba, active, knobs, passes=passes, sub=sub)
    o = ws.make_oracle(conf, active=active, user_group=True)
    nhot = ws.simulate_blocks(o, ba, NP, 3, passes, sub=sub, user_bias=user_bias)[0]
    _same(_views(t), {name: o.view(name) for name in VIEWS})
    assert (nhot > 0) == hot and t.counter(35) == nhot, (nhot, t.counter(35))
    assert t.counter(33) + t.counter(34) == 3 * passes and (not hot or t.counter(34) > 0)
    return t, ds


def _slot_range(ba, s=None):
    """the fewest and the most slots a shared id meets in one of the 3 windows"""
    blocks = ba.to_blocks()
    lo, hi = 1 << 30, 0
    for b0, b1 in ws.block_cuts(ba, 3):
        c = ws.slot_counts(blocks[b0:b1], NP)
        vals = [c.get(NP + j, 0) for j in range(NS)] if s is None else [c.get(s, 0)]
        lo, hi = min(lo, min(vals)), max(hi, max(vals))
    return lo, hi


# (k, sub, active_type, reg_method, extra keys, generator options)
CASES = [
    (1, 5, 0, 0, (), dict(positions=("first",))),
    (7, 3, 0, 1, (("user_nonnegative", "1"),), dict(positions=("middle",), uvals=True)),
    (16, 1, 2, 3, (), dict(positions=("last",))),
    (64, 12, 0, 0, (), dict(uvals=True)),
    (64, 3, 3, 1, (("no_user_bias", "1"),), dict(uvals=True)),
    (64, 5, 0, 0, (), dict(uvals="all", per_row=True, min_shared=0)),
    (100, 12, 0, 0, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(uvals=True)),
    (128, 5, 0, 2, SPLIT, dict(uvals=True)),
    (128, 12, 2, 0, (("scale_lr_ufeedback", "0.5"), ("wd_user_bias", "0.01")), dict(positions=("middle", "last"), per_row=True)),
    (192, 3, 0, 3, SPLIT, dict(uvals="all")),
    (256, 12, 3, 2, (), dict(uvals=True, positions=("first", "last"))),
    (256, 1, 0, 0, (("no_user_bias", "1"), ("scale_lr_ufeedback", "2")), dict(uvals=True, per_row=True)),
]


@pytest.mark.parametrize("k,sub,active,reg,extra,opts", CASES)
def test_hot_shared_rows_equal_the_checker(k, sub, active, reg, extra, opts):
    """widths 1 .. 256 (k = 256: 4 lane groups per round), links 0 / 2 / 3, reg_method 0 - 3, no_user_bias, nonnegative users, decay ranges that split
    the shared ids, the feedback knobs, non-unit values (private ones too), the hot entry before / between / after the private one, sections
    per block and per row, START .. END spans"""
    conf = _conf(k, active, reg, extra)
    opts = dict(dict(min_shared=0, max_shared=3) if sub == 12 else dict(min_shared=1, max_shared=4), **opts)
    ba = BlockArrays.from_blocks(_blocks(k + reg, binary=active != 0, **opts))
    assert {int(x) for x in ba.extend_tag} == {TAG_DEFAULT, TAG_START, TAG_MIDDLE, TAG_END}
    lo, hi = _slot_range(ba)
    assert (lo <= sub < hi) if sub == 12 else sub < lo, (lo, hi)   # sub 12 mixes hot and cold rows, sub <= 5 makes every shared id hot
    _against_checker(conf, ba, sub, active, user_bias=dict(extra).get("no_user_bias") != "1")


def test_a_global_entry_per_row():
    conf = _conf(128, ng=4)
    ba = BlockArrays.from_blocks(_blocks(22, min_shared=1, max_shared=2, num_global=4, uvals=True))
    _against_checker(conf, ba, 5)


def test_a_unit_of_150_rows_in_sub_steps_of_40():
    """k = 64 with sub-steps of 40: a shared id of the long unit meets 169 slots in its window -- four full sub-steps and a partial one, in rounds of
    16, 16 and 8 lane groups.  (One pass: the checker replays the unit's span once per hot slot.)"""
    conf = _conf(64)
    ba = BlockArrays.from_blocks(_blocks(64, n=45, min_shared=1, max_shared=3, uvals=True, long_unit=150))
    assert _slot_range(ba)[1] == 169
    _against_checker(conf, ba, 40, passes=1)


@pytest.mark.parametrize("k,defer,sub", [(64, 0, 5), (64, 1, 5), (16, 1, 12)])
def test_long_feedback_lists_and_users_in_two_spans(k, defer, sub):
    """feedback lists of 0, 1 and 70 entries, users in several spans of one window, both values of wunit_defer_fb"""
    nf = 80
    conf = _conf(k, nf=nf)
    blocks = _blocks(64, num_fb=nf, min_shared=1, max_shared=4, uvals=True, fb_sizes=(0, 1, 70, 3))
    ba = BlockArrays.from_blocks(blocks)
    for b0, b1 in ws.block_cuts(ba, 3):
        owners = [min(int(x) for x in b.data.row(0)[4][:b.data.row(0)[2]]) for b in blocks[b0:b1] if b.extend_tag in (TAG_DEFAULT, TAG_START)]
        assert len(set(owners)) < len(owners)   # some user has two spans in this window
    _against_checker(conf, ba, sub, knobs=[("wunit_defer_fb", defer)])


@pytest.mark.parametrize("k", [16, 64])
def test_where_no_row_is_hot_the_knob_changes_no_bit(k):
    """blocks without shared ids, and a sub-step above every slot count: the bits of the knob off, which are the plain window step's; counter 35 stays 0"""
    conf = _conf(k)
    plain = BlockArrays.from_blocks(_blocks(5, max_shared=0))
    a, _ = _run(conf, plain, sub=None)
    b, _ = _run(conf, plain, sub=3)
    _same(_views(a), _views(b))
    assert b.counter(35) == 0 and b.counter(34) == 0
    ba = BlockArrays.from_blocks(_blocks(k, min_shared=1, max_shared=4, uvals=True))
    hi = _slot_range(ba)[1]
    off, _ = _run(conf, ba, sub=0)
    on, _ = _against_checker(conf, ba, hi, hot=False)
    _same(_views(off), _views(on))
    o = ws.make_oracle(conf, user_group=True)
    ws.simulate_blocks(o, ba, NP, 3, 2)
    _same(_views(off), {name: o.view(name) for name in VIEWS})
    nokey, _ = _run(conf, plain, extra=[("amd:step", "minibatch")], sub=3)   # a trainer without amd:shared_user_from
    _same(_views(a), _views(nokey))


@pytest.mark.parametrize("k,sub,per_row", [(16, 3, True), (64, 12, False), (192, 5, False)])
def test_scoring_equals_predict_block_and_leaves_training_alone(k, sub, per_row):
    conf = _conf(k)
    blocks = _blocks(k, min_shared=0 if per_row else 1, max_shared=4, uvals=True, per_row=per_row)
    ba = BlockArrays.from_blocks(blocks)
    t, ds = _run(conf, ba, passes=1, sub=sub)
    assert t.counter(35) > 0
    got = t.predict_dataset(ds)
    want = np.concatenate([t.predict_block(b) for b in blocks])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ss, cnt = t.eval_dataset(ds)
    ref = float(np.sum((got - ba.row_label).astype(np.float64) ** 2))
    assert cnt == ba.num_row and abs(ss - ref) <= 1e-9 * ss
    t.train_dataset(ds)          # train -> score -> train ...
    t.synchronize()
    u, _ = _run(conf, ba, passes=2, sub=sub)   # ... equals train -> train
    _same(_views(t), _views(u))


def _dense_blocks(seed, nblocks=3000, nu=300, ns=4, ni=200):
    """every row carries one of `ns` bucket ids: each bucket is met by 1 / ns of all rows"""
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(nblocks):
        u = int(rng.integers(0, nu))
        rows = [(float(rng.integers(1, 6)), [], [(u, 1.0), (nu + u % ns, 1.0)], [(int(rng.integers(0, ni)), 1.0)]) for _ in range(int(rng.integers(1, 8)))]
        fbi = np.sort(rng.choice(ni, size=3, replace=False)).astype(np.uint32)
        blocks.append(PlusBlock(fbi, np.full(3, 3 ** -0.5, np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    return BlockArrays.from_blocks(blocks)


def _pass_counts(ba, nu, ns, ni):
    """what the rule of wseq_from_blocks reads: the pass's updates of every item row and shared user row, the feedback rows' mass"""
    rows = ba.rows()
    ci = np.zeros(ni, np.int64)
    cs = np.zeros(ns, np.int64)
    for r in range(ba.num_row):
        _, ng, nuu, _, idx, _ = rows.row(r)
        for x in idx[ng:ng + nuu]:
            if x >= nu:
                cs[int(x) - nu] += 1
        for x in idx[ng + nuu:]:
            ci[int(x)] += 1
    mass = np.zeros(ni)
    for b in ba.to_blocks():
        for f, v in zip(b.index_ufeedback, b.value_ufeedback):
            mass[int(f)] += b.data.num_row * abs(float(v))
    return ci, cs, mass


@pytest.mark.parametrize("sub,cap", [(12, 512), (8, 128), (12, 64)])
def test_the_default_window_rule_on_dense_buckets(sub, cap):
    """no amd:window: with the knob on, a dense bucket row no longer sets the window count by its 12 updates per window -- the rule of section 6k with
    window_block_max as the cap"""
    nu, ns, ni = 300, 4, 200
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu + ns, num_item=ni, num_factor=32, num_ufeedback=ni) + SVDPP
    ba = _dense_blocks(3)
    key = [("amd:step", "minibatch"), ("amd:shared_user_from", nu)]
    off = _trainer(conf, extra=key)
    d0 = off.dataset_from_blocks(ba)
    t = _trainer(conf, extra=key, knobs=[("window_block_sub", sub), ("window_block_max", cap)])
    ds = t.dataset_from_blocks(ba)
    ci, cs, mass = _pass_counts(ba, nu, ns, ni)
    want = wr.blocks(ba.num_row, ba.num_block, ci, (), cs, mass, shared_lane=(sub, cap))
    assert ds.kind == 8 and ds.num_batches == want and want < d0.num_batches, (ds.num_batches, want, d0.num_batches)
    t.train_dataset(ds)
    t.synchronize()
    assert t.counter(35) > 0 and t.counter(34) == ds.num_batches


def _one(users, tag=TAG_DEFAULT, fb=(1, 2), n=1):
    fbi = np.array(fb, np.uint32)
    return PlusBlock(fbi, np.full(len(fb), 0.5, np.float32), CSRData.from_rows([(3.0, [], u, [(2 + j, 1.0)]) for j in range(n) for u in users]), tag)


def test_refusals_name_the_knob():
    conf = _conf(8)
    shared = [_one([[(1, 1.0), (NP + 3, 1.0)]], n=3)]   # id NP + 3 meets three slots
    b = _trainer(conf, 0, MB + [("amd:contrib", "bf16")], [("window_block_sub", 2)])
    with pytest.raises(sa.SvdfError, match=r"window_block_sub > 0 .*amd:contrib = fp32"):
        b.dataset_from_blocks(shared)
    i = _trainer(conf, 0, MB, [("window_block_sub", 2), ("wunit_inplace", 0)])
    with pytest.raises(sa.SvdfError, match=r"window_block_sub > 0 .*wunit_inplace = 1"):
        i.dataset_from_blocks(shared)
    i.set_knob("window_block_sub", 3)   # ... once a row is hot: none is at 3
    i.dataset_from_blocks(shared)
    w = _trainer(conf, 0, [("amd:shared_user_from", NP)], [("window_block_sub", 2)])
    with pytest.raises(sa.SvdfError, match=r"svdf_dataset_window_from_blocks.*window_block_sub > 0 .*one-GPU window sequence"):
        w.dataset_window_from_blocks(BlockArrays.from_blocks([_one([[(1, 1.0)]])]))
    g = sa.Trainer(1, 0)
    g.set_param("amd:gpus", "2")
    with pytest.raises(sa.SvdfError, match=r"window_block_sub > 0 .*amd:gpus > 1"):
        g.set_knob("window_block_sub", 2)
    for knob, lo, hi in (("window_block_sub", -1, 4097), ("window_block_max", 0, None)):
        for v in (lo, hi):
            if v is not None:
                with pytest.raises(sa.SvdfError, match=knob):
                    _trainer(conf, 0, MB).set_knob(knob, v)
    # the csr lanes' knobs stay refused with user-group trainers, next to the new knob too
    for knob in ("window_shared_sub", "window_item_sub"):
        s = _trainer(conf, 0, MB, [(knob, 4), ("window_block_sub", 2)])
        with pytest.raises(sa.SvdfError, match=knob + ".*not supported with user-group"):
            s.dataset_from_blocks(shared)


def test_a_sequence_built_with_another_value_is_refused():
    conf = _conf(16)
    ba = BlockArrays.from_blocks(_blocks(16, min_shared=1, max_shared=4))
    t = _trainer(conf, 0, MB + _window_key(ba), [("window_block_sub", 5)])
    ds = t.dataset_from_blocks(ba)
    t.train_dataset(ds)
    t.set_knob("window_block_sub", 3)
    with pytest.raises(sa.SvdfError, match="built with another window_block_sub"):
        t.train_dataset(ds)
    t.set_knob("window_block_sub", 0)
    with pytest.raises(sa.SvdfError, match="built with another window_block_sub"):
        t.train_dataset(ds)
    t.set_knob("window_block_sub", 5)
    t.train_dataset(ds)
    t.synchronize()
    u, _ = _run(conf, ba, sub=5)
    _same(_views(t), _views(u))


def test_the_staged_route_and_auto_keep_the_exact_pass_with_the_knob_on():
    conf = _conf(64)
    blocks = _blocks(9, min_shared=1, max_shared=4, uvals=True)

    def feed(t):
        for b in blocks:
            t.update_block(b)
        t.finish_round()
        t.synchronize()
        return t
    t = feed(_trainer(conf, 0, MB, [("stage_window", 120), ("window_block_sub", 5)]))
    assert t.counter(30) == 0 and t.counter(31) >= 2 and t.counter(34) == 0 and t.counter(35) == 0
    x = feed(_trainer(conf, 0, [], [("stage_window", 120)]))   # the default step
    _same(_views(t), _views(x))
    nu, ns, ni = 300, 4, 200
    dconf = cases.conf_with(cases.BASICMF_CONF, num_user=nu + ns, num_item=ni, num_factor=32, num_ufeedback=ni) + SVDPP
    ba = _dense_blocks(3, nblocks=4000)
    a = _trainer(dconf, extra=[("amd:step", "auto"), ("amd:shared_user_from", nu)], knobs=[("window_block_sub", 12)])
    ds = a.dataset_from_blocks(ba)
    assert a.counter(16) == 3 and ds.kind != 8


def test_the_buffer_file_route_equals_the_block_route(tmp_path):
    from svdfeature_amd import data as D
    conf = _conf(64)
    blocks = _blocks(21, min_shared=1, max_shared=3, split_every=3)
    path = str(tmp_path / "shared.ug")
    D.write_ugroup_buffer(path, blocks)
    ba = BlockArrays.from_blocks(blocks)
    a, _ = _run(conf, ba, sub=5)
    b = _trainer(conf, 0, MB + _window_key(ba), [("window_block_sub", 5)])
    ds = b.dataset_from_buffer_file(path, user_group=True)
    assert ds.kind == 8 and ds.num_batches == 3
    for _ in range(2):
        b.train_dataset(ds)
    b.synchronize()
    _same(_views(a), _views(b))
    assert a.counter(35) == b.counter(35) > 0


def test_short_fuzz_run():
    import fuzz_block_hot
    assert fuzz_block_hot.run(iters=10, seed=7) == 0

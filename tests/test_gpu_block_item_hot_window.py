"""Ordered sub-steps for hot item rows of user-group (SVD++) blocks in the one-GPU window step (knobs `window_block_item_sub`,
`window_block_item_max` on a format_type 1 trainer, with or without `amd:shared_user_from`; svdf_wunit.cpp, svdf_k_wunit.hip:
k_wunit_walk<LPI, true, true> and k_wunit_apply_hot<LPI, true, true>).  An item row with more than `window_block_item_sub`
slots in a window is applied in file order, that many slots at a time, every slot computed from the span state the walk held when it reached the
data row (private row and bias, tmp_ufeedback and its bias).  All seven views must equal the checker of tests/window_sim.py -- the pinned
C port of SVDPPFeature::update with every hot slot's span replayed from its start -- bit for bit, and counters 35 / 36 the checker's counts of
hot user rows / hot item rows."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

pytestmark = pytest.mark.gpu

NP, NS, NI, NF = 60, 8, 8, 40      # private users, shared user ids, items (few: they are hot), feedback ids: otherwise the shape of tests/test_gpu_block_hot_window.py
NU = NP + NS
VIEWS = ws.VIEWS
SVDPP = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
MB = [("amd:step", "minibatch")]
SHARED = MB + [("amd:shared_user_from", NP)]
SPLIT = (("ip:wd", "0.01"), ("ip:bound", "3"), ("ip:wd", "0.003"), ("ip:bound", str(NI)))   # wd_item ranges that split the items


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


def _conf(k, active=0, reg=0, extra=(), nf=NF, ng=0, ni=NI):
    c = cases.conf_with(cases.BASICMF_CONF, num_user=NU, num_item=ni, num_global=ng, num_factor=k, num_ufeedback=nf, reg_method=reg,
                        active_type=active, learning_rate="0.01", wd_global="0.002") + SVDPP + list(extra)
    return cases.conf_with(c, base_score="0.5") if active else c


def _items(blocks, seed, ni=NI, two=False, vals=False, to_zero=0.0):
    """the generator's blocks with their item entries redrawn: non-unit values, a second item entry per row, a share of the rows sent to item 0"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for b in blocks:
        rows = []
        for r in range(b.data.num_row):
            label, ng, nu, _, idx, val = b.data.row(r)
            i = 0 if rng.random() < to_zero else int(idx[ng + nu])
            v = lambda: float(rng.choice([1.0, 0.5, 2.0, 0.25])) if vals else 1.0   # noqa: E731
            it = [(i, v())]
            if two:
                it.append(((i + 1 + int(rng.integers(0, ni - 1))) % ni, v()))
                it = it[::-1] if rng.random() < 0.5 else it
            rows.append((float(label), [(int(x), float(y)) for x, y in zip(idx[:ng], val[:ng])],
                         [(int(x), float(y)) for x, y in zip(idx[ng:ng + nu], val[ng:ng + nu])], it))
        out.append(PlusBlock(b.index_ufeedback, b.value_ufeedback, CSRData.from_rows(rows), b.extend_tag))
    return out


def _blocks(seed, n=75, ni=NI, items=None, **kw):
    kw.setdefault("max_shared", 0)   # plain SVD++ blocks: one user entry per row
    blocks = ws.shared_blocks(np.random.default_rng(seed), n, NP, NS, ni, kw.pop("num_fb", NF), **kw)
    return _items(blocks, seed, ni, **items) if items else blocks


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


def _run(conf, ba, active=0, knobs=(), passes=2, extra=MB, isub=0, sub=0):
    knobs = list(knobs) + ([("window_block_item_sub", isub)] if isub is not None else []) + ([("window_block_sub", sub)] if sub else [])
    t = _trainer(conf, active, list(extra) + _window_key(ba), knobs)
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches == 3, (ds.kind, ds.num_batches)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    return t, ds


def _against_checker(conf, ba, isub, active=0, knobs=(), user_bias=True, hot=True, passes=2, extra=MB, sub=0):
    """2 passes of 3 windows against window_sim.step_blocks; counters 35 / 36 = the checker's hot user rows / hot item rows"""
    t, ds = _run(conf, ba, active, knobs, passes=passes, extra=extra, isub=isub, sub=sub)
    o = ws.make_oracle(conf, active=active, user_group=True)
    B = NP if any(k == "amd:shared_user_from" for k, _ in extra) else NU
    nuh, nih = ws.simulate_blocks(o, ba, B, 3, passes, isub=isub, sub=sub, user_bias=user_bias)
    assert all(np.isfinite(v).all() for v in _views(t).values() if v is not None)
    _same(_views(t), {name: o.view(name) for name in VIEWS})
    assert (nih > 0) == hot and t.counter(36) == nih and t.counter(35) == nuh, (nuh, nih, t.counter(35), t.counter(36))
    return t, ds


def _slot_range(ba, item=None):
    """the fewest and the most slots an item meets in one of the 3 windows"""
    blocks = ba.to_blocks()
    lo, hi = 1 << 30, 0
    for b0, b1 in ws.block_cuts(ba, 3):
        c = ws.block_item_slot_counts(blocks[b0:b1])
        vals = [c.get(j, 0) for j in range(NI)] if item is None else [c.get(item, 0)]
        lo, hi = min(lo, min(vals)), max(hi, max(vals))
    return lo, hi


# (k, isub, active_type, reg_method, extra keys, generator options, item options)
CASES = [
    (1, 5, 0, 0, (), dict(), None),
    (5, 3, 0, 1, (("user_nonnegative", "1"),), dict(), dict(vals=True)),
    (16, 5, 2, 3, (), dict(), None),
    (64, 12, 0, 0, (), dict(), dict(vals=True)),
    (64, 3, 3, 1, (("no_user_bias", "1"),), dict(), dict(vals=True)),
    (64, 5, 0, 0, (), dict(), dict(two=True, vals=True)),
    (100, 12, 0, 0, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(), None),
    (128, 1, 0, 2, SPLIT, dict(), dict(vals=True)),   # (reg_method 2 projects every change onto the ball: 5 changes of a row against one value overshoot, lane or not)
    (128, 12, 2, 0, (("scale_lr_ufeedback", "0.5"), ("wd_item_bias", "0.01")), dict(), dict(two=True)),
    (200, 3, 0, 3, SPLIT, dict(), dict(two=True, vals=True)),
    (256, 12, 3, 1, (), dict(), None),
    (256, 1, 0, 0, (("no_user_bias", "1"), ("scale_lr_ufeedback", "2")), dict(), dict(vals=True)),
]


@pytest.mark.parametrize("k,isub,active,reg,extra,opts,items", CASES)
def test_hot_item_rows_equal_the_checker(k, isub, active, reg, extra, opts, items):
    """widths 1 .. 256 (every lane-group size, ragged widths), links 0 / 2 / 3, reg_method 0 - 3, no_user_bias, nonnegative users, item decay ranges that
    split the items, the feedback knobs, non-unit item values, two item entries per row (both hot at sub <= 5), START .. END spans"""
    conf = _conf(k, active, reg, extra)
    ba = BlockArrays.from_blocks(_blocks(k + reg, binary=active != 0, items=items, **opts))
    assert {int(x) for x in ba.extend_tag} == {TAG_DEFAULT, TAG_START, TAG_MIDDLE, TAG_END}
    lo, hi = _slot_range(ba)
    two = bool(items and items.get("two"))
    assert (lo <= isub < hi) if isub == 12 and not two else isub < lo, (lo, hi)   # sub 12 mixes hot and cold items, sub <= 5 makes every item hot
    _against_checker(conf, ba, isub, active, user_bias=dict(extra).get("no_user_bias") != "1")


def test_a_global_entry_per_row():
    conf = _conf(128, ng=4)
    ba = BlockArrays.from_blocks(_blocks(22, num_global=4, items=dict(vals=True)))
    _against_checker(conf, ba, 5)


def test_a_unit_of_150_rows_in_sub_steps_of_40():
    """k = 64 with sub-steps of 40: item 0 meets more than 80 slots in the long unit's window -- full sub-steps and a partial one, in rounds of
    16, 16 and 8 lane groups.  (One pass: the checker replays the unit's span once per hot slot.)"""
    conf = _conf(64)
    ba = BlockArrays.from_blocks(_blocks(64, n=45, long_unit=150, items=dict(to_zero=0.5)))
    hi = _slot_range(ba, 0)[1]
    assert hi > 80 and hi % 40 != 0, hi
    _against_checker(conf, ba, 40, passes=1)


@pytest.mark.parametrize("k,defer,isub", [(64, 0, 5), (64, 1, 5), (16, 1, 12)])
def test_long_feedback_lists_and_users_in_two_spans(k, defer, isub):
    """feedback lists of 0, 1 and 70 entries, users in several spans of one window, both values of wunit_defer_fb"""
    nf = 80
    conf = _conf(k, nf=nf)
    blocks = _blocks(64, num_fb=nf, fb_sizes=(0, 1, 70, 3), items=dict(vals=True))
    ba = BlockArrays.from_blocks(blocks)
    for b0, b1 in ws.block_cuts(ba, 3):
        owners = [int(b.data.row(0)[4][b.data.row(0)[1]]) for b in blocks[b0:b1] if b.extend_tag in (TAG_DEFAULT, TAG_START)]
        assert len(set(owners)) < len(owners)   # some user has two spans in this window
    _against_checker(conf, ba, isub, knobs=[("wunit_defer_fb", defer)])


@pytest.mark.parametrize("k,isub,sub,opts", [
    (64, 5, 5, dict(min_shared=1, max_shared=3, uvals=True)),
    (16, 12, 3, dict(min_shared=1, max_shared=4, uvals="all", per_row=True)),
    (128, 3, 0, dict(min_shared=0, max_shared=3, uvals=True)),
])
def test_blocks_with_shared_user_ids_and_both_lanes(k, isub, sub, opts):
    """amd:shared_user_from with window_block_sub on at once: a data row has a hot user entry and a hot item entry, one slot to each, each evaluated
    with the other at its window-start value (sub = 0: shared rows cold, items hot)"""
    conf = _conf(k)
    ba = BlockArrays.from_blocks(_blocks(k, items=dict(vals=True), **opts))
    t, _ = _against_checker(conf, ba, isub, extra=SHARED, sub=sub)
    assert (t.counter(35) > 0) == (sub > 0) and t.counter(34) == 6


@pytest.mark.parametrize("k", [16, 64])
def test_where_no_item_is_hot_the_knob_changes_no_bit(k):
    """a sub-step above every slot count: the bits of the knob off and of the knob unset, which are the plain window step's; counter 36 stays 0"""
    conf = _conf(k)
    ba = BlockArrays.from_blocks(_blocks(k))
    hi = _slot_range(ba)[1]
    assert hi <= 128
    unset, _ = _run(conf, ba, isub=None)
    off, _ = _run(conf, ba, isub=0)
    on, _ = _against_checker(conf, ba, hi, hot=False)
    _same(_views(unset), _views(off))
    _same(_views(off), _views(on))
    o = ws.make_oracle(conf, user_group=True)
    ws.simulate_blocks(o, ba, NU, 3, 2)
    _same(_views(off), {name: o.view(name) for name in VIEWS})
    hot, _ = _run(conf, ba, isub=3)
    assert hot.counter(36) > 0
    with pytest.raises(AssertionError):
        _same(_views(off), _views(hot))


@pytest.mark.parametrize("k,isub,two", [(16, 3, True), (64, 12, False), (200, 5, False)])
def test_scoring_equals_predict_block_and_leaves_training_alone(k, isub, two):
    conf = _conf(k)
    blocks = _blocks(k, items=dict(two=two, vals=True))
    ba = BlockArrays.from_blocks(blocks)
    t, ds = _run(conf, ba, passes=1, isub=isub)
    assert t.counter(36) > 0
    got = t.predict_dataset(ds)
    want = np.concatenate([t.predict_block(b) for b in blocks])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ss, cnt = t.eval_dataset(ds)
    ref = float(np.sum((got - ba.row_label).astype(np.float64) ** 2))
    assert cnt == ba.num_row and abs(ss - ref) <= 1e-9 * ss
    t.train_dataset(ds)          # train -> score -> train ...
    t.synchronize()
    u, _ = _run(conf, ba, passes=2, isub=isub)   # ... equals train -> train
    _same(_views(t), _views(u))


def _zipf_blocks(seed, nblocks=3000, nu=300, ni=200, nf=2000, s=0.7):
    """SVD++ blocks whose items are drawn Zipf(s)"""
    rng = np.random.default_rng(seed)
    p = np.arange(1, ni + 1, dtype=np.float64) ** -s
    p /= p.sum()
    blocks = []
    for _ in range(nblocks):
        u = int(rng.integers(0, nu))
        rows = [(float(rng.integers(1, 6)), [], [(u, 1.0)], [(int(rng.choice(ni, p=p)), 1.0)]) for _ in range(int(rng.integers(1, 8)))]
        fbi = np.sort(rng.choice(nf, size=3, replace=False)).astype(np.uint32)
        blocks.append(PlusBlock(fbi, np.full(3, 3 ** -0.5, np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    return BlockArrays.from_blocks(blocks)


def _pass_counts(ba, ni, nf):
    """what the rule of wseq_from_blocks reads: the pass's updates of every item row, the feedback rows' mass"""
    rows = ba.rows()
    ci = np.zeros(ni, np.int64)
    for r in range(ba.num_row):
        _, ng, nuu, _, idx, _ = rows.row(r)
        for x in idx[ng + nuu:]:
            ci[int(x)] += 1
    mass = np.zeros(nf)
    for b in ba.to_blocks():
        for f, v in zip(b.index_ufeedback, b.value_ufeedback):
            mass[int(f)] += b.data.num_row * abs(float(v))
    return ci, mass


@pytest.mark.parametrize("sub,cap", [(12, 512), (64, 128), (24, 2048)])
def test_the_default_window_rule_on_zipf_items(sub, cap):
    """no amd:window: with the knob on, a Zipf-popular item no longer sets the window count through window_per_target_max -- the rule of section 6m
    with window_block_item_max as the cap"""
    nu, ni, nf = 300, 200, 2000
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32, num_ufeedback=nf) + SVDPP
    ba = _zipf_blocks(3)
    off = _trainer(conf, extra=MB)
    d0 = off.dataset_from_blocks(ba)
    ci, mass = _pass_counts(ba, ni, nf)
    assert d0.num_batches == wr.blocks(ba.num_row, ba.num_block, ci, fb_mass=mass)
    t = _trainer(conf, extra=MB, knobs=[("window_block_item_sub", sub), ("window_block_item_max", cap)])
    ds = t.dataset_from_blocks(ba)
    want = wr.blocks(ba.num_row, ba.num_block, ci, fb_mass=mass, item_lane=(sub, cap))
    assert ds.kind == 8 and ds.num_batches == want, (ds.num_batches, want, d0.num_batches)
    assert want < d0.num_batches or sub > 24   # (sub-steps above window_per_target: the mean over entries asks for the windows, not the cap)
    t.train_dataset(ds)
    t.synchronize()
    assert t.counter(36) > 0 and all(np.isfinite(t.view(name)).all() for name in ("W_item", "i_bias", "W_user"))
    w = _trainer(conf, extra=MB + [("amd:window", 4000)], knobs=[("window_block_item_sub", sub), ("window_block_item_max", cap)])
    assert w.dataset_from_blocks(ba).num_batches == -(-ba.num_row // 4000)   # amd:window overrides the rule


def _one(user, tag=TAG_DEFAULT, fb=(1, 2), n=1, item=2):
    fbi = np.array(fb, np.uint32)
    return PlusBlock(fbi, np.full(len(fb), 0.5, np.float32), CSRData.from_rows([(3.0, [], [(user, 1.0)], [(item, 1.0)]) for _ in range(n)]), tag)


def test_refusals_name_the_knob():
    conf = _conf(8)
    hot = [_one(1, n=3)]   # item 2 meets three slots
    b = _trainer(conf, 0, MB + [("amd:contrib", "bf16")], [("window_block_item_sub", 2)])
    with pytest.raises(sa.SvdfError, match=r"window_block_item_sub > 0 .*amd:contrib = fp32"):
        b.dataset_from_blocks(hot)
    i = _trainer(conf, 0, MB, [("window_block_item_sub", 2), ("wunit_inplace", 0)])
    with pytest.raises(sa.SvdfError, match=r"window_block_item_sub > 0 .*wunit_inplace = 1"):
        i.dataset_from_blocks(hot)
    i.set_knob("window_block_item_sub", 3)   # ... once a row is hot: none is at 3
    i.dataset_from_blocks(hot)
    w = _trainer(conf, 0, [], [("window_block_item_sub", 2)])
    with pytest.raises(sa.SvdfError, match=r"svdf_dataset_window_from_blocks.*window_block_item_sub > 0 .*one-GPU window sequence"):
        w.dataset_window_from_blocks(BlockArrays.from_blocks([_one(1)]))
    g = sa.Trainer(1, 0)
    g.set_param("amd:gpus", "2")
    with pytest.raises(sa.SvdfError, match=r"window_block_item_sub > 0 .*amd:gpus > 1"):
        g.set_knob("window_block_item_sub", 2)
    wide = _trainer(_conf(300), 0, MB, [("window_block_item_sub", 2)])
    with pytest.raises(sa.SvdfError, match=r"window_block_item_sub > 0 .* needs num_factor <= 256"):
        wide.dataset_from_blocks(hot)
    wide.set_knob("window_block_item_sub", 0)
    wide.dataset_from_blocks(hot)
    for knob, lo, hi in (("window_block_item_sub", -1, 129), ("window_block_item_max", 0, None)):
        for v in (lo, hi):
            if v is not None:
                with pytest.raises(sa.SvdfError, match=knob):
                    _trainer(conf, 0, MB).set_knob(knob, v)
    # the csr lane's knob stays refused with user-group trainers, next to the new knob too
    s = _trainer(conf, 0, MB, [("window_item_sub", 4), ("window_block_item_sub", 2)])
    with pytest.raises(sa.SvdfError, match="window_item_sub.*not supported with user-group"):
        s.dataset_from_blocks(hot)
    # a random-order trainer does not know the lane: the knob is without effect there
    r = sa.Trainer(0, 0)
    r.seed(10)
    for k_, v_ in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=NI, num_factor=8) + [("amd:step", "minibatch")]:
        r.set_param(k_, str(v_))
    r.init_model()
    r.init_trainer()
    r.set_knob("window_block_item_sub", 2)
    d = CSRData.from_rows([(3.0, [], [(j % 5, 1.0)], [(2 + j % 2, 1.0)]) for j in range(12)])
    ds = r.dataset_from_csr(d)
    r.train_dataset(ds)
    r.synchronize()
    assert r.counter(36) == 0


def test_a_sequence_built_with_another_value_is_refused():
    conf = _conf(16)
    ba = BlockArrays.from_blocks(_blocks(16))
    t = _trainer(conf, 0, MB + _window_key(ba), [("window_block_item_sub", 5)])
    ds = t.dataset_from_blocks(ba)
    t.train_dataset(ds)
    t.set_knob("window_block_item_sub", 3)
    with pytest.raises(sa.SvdfError, match="built with another window_block_item_sub"):
        t.train_dataset(ds)
    t.set_knob("window_block_item_sub", 0)
    with pytest.raises(sa.SvdfError, match="built with another window_block_item_sub"):
        t.train_dataset(ds)
    t.set_knob("window_block_item_sub", 5)
    t.train_dataset(ds)
    t.synchronize()
    u, _ = _run(conf, ba, isub=5)
    _same(_views(t), _views(u))


def test_the_staged_route_equals_the_resident_sequence_chunk_by_chunk():
    """svdf_update_block under amd:step = minibatch calls wseq_from_blocks per chunk: it follows the knob"""
    from test_gpu_staged_window import _block_cuts
    conf = _conf(64)
    blocks = _blocks(9, n=110, items=dict(vals=True))
    window = 150
    cuts = _block_cuts(blocks, window)
    assert len(cuts) >= 3
    assert all(max(ws.block_item_slot_counts(blocks[a:b]).values()) > 5 for a, b in cuts)
    make = lambda isub: _trainer(conf, 0, MB, [("stage_window", window), ("window_block_item_sub", isub)])   # noqa: E731

    def feed(t):
        for b in blocks:
            t.update_block(b)
        t.finish_round()
        t.synchronize()
        return t
    t, z = feed(make(5)), feed(make(0))
    r = make(5)
    for a, b in cuts:
        ds = r.dataset_from_blocks(BlockArrays.from_blocks(blocks[a:b]))
        assert ds.kind == 8
        r.train_dataset(ds)
        ds.close()
    r.synchronize()
    _same(_views(t), _views(r))
    assert t.counter(30) == len(cuts) and t.counter(31) == 0 and t.counter(36) == r.counter(36) > 0 and z.counter(36) == 0
    with pytest.raises(AssertionError):
        _same(_views(t), _views(z))


def test_the_buffer_file_route_equals_the_block_route(tmp_path):
    from svdfeature_amd import data as D
    conf = _conf(64)
    blocks = _blocks(21, split_every=3, items=dict(vals=True))
    path = str(tmp_path / "items.ug")
    D.write_ugroup_buffer(path, blocks)
    ba = BlockArrays.from_blocks(blocks)
    a, _ = _run(conf, ba, isub=5)
    b = _trainer(conf, 0, MB + _window_key(ba), [("window_block_item_sub", 5)])
    ds = b.dataset_from_buffer_file(path, user_group=True)
    assert ds.kind == 8 and ds.num_batches == 3
    for _ in range(2):
        b.train_dataset(ds)
    b.synchronize()
    _same(_views(a), _views(b))
    assert a.counter(36) == b.counter(36) > 0


def test_short_fuzz_run():
    import fuzz_block_item_hot
    assert fuzz_block_item_hot.run(iters=10, seed=7) == 0

"""Shared user ids on user-group (SVD++) blocks in the one-GPU window step (`amd:shared_user_from = B` on a format_type 1 trainer; svdf_wunit.cpp,
svdf_k_wunit.hip, svdf_k_wave.hip): every row of a DEFAULT block or START..END span carries the unit's private id (< B) and any
number of shared ids (>= B: region, device class ...), which are read as of the window start and move once per window, like item and feedback rows.
Every view must equal the checker of tests/window_sim.py -- the pinned C port of SVDPPFeature::update fed row by row on (the private state the
walk holds, the window-start shared rows), shared changes summed per target in file order -- bit for bit.  Windows whose segments carry ONE user
section each (attributes of the user) run one wave per unit with the section's rows in registers under knob wunit_fast = 3 (counter 33); everything else
with shared entries, and every such window by default, runs the general lane-group kernel (counter 34)."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_rule as wr
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

pytestmark = pytest.mark.gpu

NP, NS, NI, NF = 60, 8, 40, 40      # private users, shared user ids (B = NP), items, feedback ids
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


def _seq(t, ba, windows=3):
    """the sequence cut into `windows` windows through amd:window (rows per window)"""
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches == windows, (ds.kind, ds.num_batches)
    return ds


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


def _run(conf, ba, active=0, knobs=(), passes=2, extra=MB):
    t = _trainer(conf, active, list(extra) + _window_key(ba), knobs)
    ds = _seq(t, ba)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    return t, ds


def _against_checker(conf, ba, active=0, knobs=(), wave=None, user_bias=True):
    """2 passes of 3 windows; wave: True = every window in the wave form, False = every window in the general kernel, None = not asserted"""
    t, ds = _run(conf, ba, active, list(knobs) + ([("wunit_fast", 3)] if wave else []))   # (the wave form is opt-in: knob wunit_fast = 3)
    o = ws.make_oracle(conf, active=active, user_group=True)
    ws.simulate_blocks(o, ba, NP, 3, 2, user_bias=user_bias)
    _same(_views(t), {name: o.view(name) for name in VIEWS})
    c33, c34 = t.counter(33), t.counter(34)
    if wave is True:
        assert (c33, c34) == (6, 0), (c33, c34)
    elif wave is False:
        assert (c33, c34) == (0, 6), (c33, c34)
    return t, ds


# (k, active_type, reg_method, extra keys, generator options): user attributes -- one section per block, 1 .. 4 shared ids around the private one
UNIFORM = [
    (1, 0, 0, (), dict(positions=("first",))),
    (7, 0, 1, (("user_nonnegative", "1"),), dict(positions=("middle",), uvals=True)),
    (16, 2, 3, (), dict(positions=("last",))),
    (64, 0, 0, (), dict(uvals=True)),
    (64, 3, 1, (("no_user_bias", "1"),), dict(uvals=True)),
    (100, 0, 0, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(uvals=True)),
    (128, 0, 2, SPLIT, dict(uvals=True)),
    (128, 2, 0, (("scale_lr_ufeedback", "0.5"), ("wd_user_bias", "0.01")), dict(positions=("middle", "last"))),
    (192, 0, 3, SPLIT, dict(uvals=True)),
    (256, 3, 2, (), dict(uvals=True, positions=("first", "last"))),
    (256, 0, 0, (("no_user_bias", "1"), ("scale_lr_ufeedback", "2")), dict(uvals=True)),
]


@pytest.mark.parametrize("k,active,reg,extra,opts", UNIFORM)
def test_user_attributes_equal_the_checker(k, active, reg, extra, opts):
    """a user's shared ids on every row of its block: the wave form at k = 64 / 128 / 192 / 256 (counter 33), the general kernel elsewhere (34)"""
    conf = _conf(k, active, reg, extra)
    ba = BlockArrays.from_blocks(_blocks(k + reg, min_shared=1, max_shared=4, binary=active != 0, **opts))
    assert {int(x) for x in ba.extend_tag} == {TAG_DEFAULT, TAG_START, TAG_MIDDLE, TAG_END}
    _against_checker(conf, ba, active, wave=k % 64 == 0, user_bias=dict(extra).get("no_user_bias") != "1")


GENERAL = [  # what sends a window with shared entries to the general kernel at a width the wave form covers
    ("five_shared_ids", 64, dict(min_shared=5, max_shared=5), 0),
    ("sections_differ_inside_a_span", 128, dict(per_row=True, max_shared=3, uvals=True), 0),
    ("non_unit_private_values", 64, dict(uvals="all", min_shared=1, max_shared=3), 0),
    ("a_global_entry_per_row", 128, dict(min_shared=1, max_shared=2, num_global=4), 4),
]


@pytest.mark.parametrize("name,k,opts,ng", GENERAL)
def test_shapes_outside_the_wave_form_take_the_general_kernel(name, k, opts, ng):
    conf = _conf(k, ng=ng)
    ba = BlockArrays.from_blocks(_blocks(len(name), **opts))
    _against_checker(conf, ba, wave=False)


@pytest.mark.parametrize("k,defer", [(64, 0), (64, 1), (128, 1), (16, 0)])
def test_long_units_long_feedback_lists_and_the_in_place_single(k, defer):
    """a unit of 150 rows (more than two 64-record blocks), feedback lists of 0, 1 and 70 entries, users in several spans of one window, and a last
    one-row block whose second shared id meets nobody else: its row and bias are applied in place"""
    nf = 80
    conf = _conf(k, nf=nf)
    blocks = _blocks(k + defer, n=45, num_fb=nf, min_shared=1, max_shared=4, uvals=True, fb_sizes=(0, 1, 70, 3), long_unit=150, single=True)
    ba = BlockArrays.from_blocks(blocks)
    assert blocks[-1].data.num_row == 1 and int((ba.feat_index == NP + NS - 1).sum()) == 1
    owners = [min(int(x) for x in b.data.row(0)[4][:b.data.row(0)[2]]) for b in blocks if b.extend_tag in (TAG_DEFAULT, TAG_START)]
    assert len(set(owners)) < len(owners)   # some user has two spans
    _against_checker(conf, ba, knobs=[("wunit_defer_fb", defer)], wave=k % 64 == 0)


@pytest.mark.parametrize("k,reg", [(64, 1), (128, 0), (256, 3)])
def test_general_kernel_and_wave_form_agree_bit_for_bit(k, reg):
    conf = _conf(k, reg=reg, extra=SPLIT)
    ba = BlockArrays.from_blocks(_blocks(3 * k, min_shared=1, max_shared=4, uvals=True))
    a, _ = _run(conf, ba, knobs=[("wunit_fast", 0)])
    b, _ = _run(conf, ba, knobs=[("wunit_fast", 3)])
    c, _ = _run(conf, ba)   # the default: the general kernel until the wave form has been measured
    assert (c.counter(33), c.counter(34)) == (0, 6)
    assert (a.counter(33), a.counter(34)) == (0, 6) and (b.counter(33), b.counter(34)) == (6, 0)
    _same(_views(a), _views(b))


@pytest.mark.parametrize("k,per_row", [(16, True), (64, False), (192, False)])
def test_scoring_equals_predict_block_and_leaves_training_alone(k, per_row):
    conf = _conf(k)
    blocks = _blocks(k, min_shared=0 if per_row else 1, max_shared=4, uvals=True, per_row=per_row)
    ba = BlockArrays.from_blocks(blocks)
    t, ds = _run(conf, ba, passes=1)
    got = t.predict_dataset(ds)
    want = np.concatenate([t.predict_block(b) for b in blocks])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ss, cnt = t.eval_dataset(ds)
    ref = float(np.sum((got - ba.row_label).astype(np.float64) ** 2))
    assert cnt == ba.num_row and abs(ss - ref) <= 1e-9 * ss
    t.train_dataset(ds)          # train -> score -> train ...
    t.synchronize()
    u, _ = _run(conf, ba, passes=2)   # ... equals train -> train
    _same(_views(t), _views(u))


def _block_cuts(blocks, window):
    """the staged route's chunks: the automatic flush waits for the open user's END once `window` rows are staged"""
    cuts, a, staged = [], 0, 0
    for j, b in enumerate(blocks):
        staged += b.data.num_row
        if staged >= window and b.extend_tag in (TAG_DEFAULT, TAG_END):
            cuts.append((a, j + 1))
            a, staged = j + 1, 0
    if a < len(blocks):
        cuts.append((a, len(blocks)))
    return cuts


def test_the_staged_update_block_route_keeps_blocks_with_shared_ids_exact(capfd):
    """until the accuracy contract has been measured on such data, staged chunks whose rows carry shared ids keep the exact flush (counter 31, one
    stderr line); blocks with one user entry per row take the step on this route with the key as without it"""
    conf = _conf(64)
    blocks = _blocks(9, min_shared=1, max_shared=4, uvals=True)
    cuts = _block_cuts(blocks, 120)
    assert len(cuts) >= 2

    def feed(t, bl=blocks):
        for b in bl:
            t.update_block(b)
        t.finish_round()
        t.synchronize()
        return t
    capfd.readouterr()
    t = feed(_trainer(conf, 0, MB, [("stage_window", 120)]))
    assert t.counter(30) == 0 and t.counter(31) == len(cuts) and t.counter(33) == 0 and t.counter(34) == 0
    assert capfd.readouterr().err.count("keep the exact pass on the staged route") == 1
    x = feed(_trainer(conf, 0, [], [("stage_window", 120)]))   # the default step
    _same(_views(t), _views(x))
    plain = _blocks(9, max_shared=0)
    got, chunks = [], []
    for extra in ([("amd:step", "minibatch")], MB):
        p = feed(_trainer(conf, 0, extra, [("stage_window", 120)]), plain)
        assert p.counter(30) >= 2 and p.counter(31) == 0   # every chunk by the window step, none kept exact
        got.append(_views(p)); chunks.append(p.counter(30))
    _same(got[0], got[1])
    assert chunks[0] == chunks[1]


def _deep_blocks(seed, nblocks=4000):
    """300 users, 4 shared ids met by a quarter of all rows each, 200 items: the exact levels are as deep as the shared ids' counts"""
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(nblocks):
        u = int(rng.integers(0, 300))
        rows = [(float(rng.integers(1, 6)), [], [(u, 1.0), (300 + u % 4, 1.0)], [(int(rng.integers(0, 200)), 1.0)]) for _ in range(int(rng.integers(1, 8)))]
        fbi = np.sort(rng.choice(200, size=3, replace=False)).astype(np.uint32)
        blocks.append(PlusBlock(fbi, np.full(3, 3 ** -0.5, np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    return BlockArrays.from_blocks(blocks)


def test_auto_keeps_blocks_with_shared_ids_on_the_exact_levels():
    """`auto` does not take the step on blocks with shared ids until its accuracy contract has been measured on them: decision 3 and the bits of the
    default step; amd:step = minibatch cuts the same data by the shared rows' term"""
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=304, num_item=200, num_factor=32, num_ufeedback=200) + SVDPP
    ba = _deep_blocks(3)
    t = _trainer(conf, extra=[("amd:step", "auto"), ("amd:shared_user_from", 300)])
    ds = t.dataset_from_blocks(ba)
    assert t.counter(16) == 3 and ds.kind != 8
    x = _trainer(conf)   # the default step
    dx = x.dataset_from_blocks(ba)
    t.train_dataset(ds); x.train_dataset(dx)
    t.synchronize(); x.synchronize()
    _same(_views(t), _views(x))
    m = _trainer(conf, extra=[("amd:step", "minibatch"), ("amd:shared_user_from", 300)])
    dm = m.dataset_from_blocks(ba)
    # the shared rows set the window count: 4 ids, at window_per_target_shared = 12 updates met per window
    counts = np.bincount(ba.feat_index[ba.feat_index >= 300] - 300, minlength=4).astype(np.float64)
    assert dm.kind == 8 and dm.num_batches == int(np.ceil(wr.met(counts, 0.0) / 12))
    m.train_dataset(dm)
    m.synchronize()
    assert m.counter(34) == dm.num_batches and m.counter(33) == 0   # k = 32: the general kernel
    b = _trainer(conf, extra=[("amd:step", "auto"), ("amd:shared_user_from", 300), ("amd:contrib", "bf16")])
    db = b.dataset_from_blocks(ba)
    assert b.counter(16) == 3 and db.kind != 8


@pytest.mark.parametrize("k", [16, 64])
def test_the_key_on_blocks_without_shared_ids_changes_no_bit(k):
    conf = _conf(k)
    ba = BlockArrays.from_blocks(_blocks(5, max_shared=0))
    got = []
    for extra in ([("amd:step", "minibatch")], MB):
        t, _ = _run(conf, ba, extra=extra)
        assert t.counter(33) == 0 and t.counter(34) == 0
        got.append(_views(t))
    _same(got[0], got[1])


def _one(users, tag=TAG_DEFAULT, fb=(1, 2)):
    fbi = np.array(fb, np.uint32)
    return PlusBlock(fbi, np.full(len(fb), 0.5, np.float32), CSRData.from_rows([(3.0, [], u, [(2, 1.0)]) for u in users]), tag)


def test_refusals_name_their_cause():
    conf = _conf(8)
    t = _trainer(conf, 0, MB)
    with pytest.raises(sa.SvdfError, match="exactly one private user entry.*two"):
        t.dataset_from_blocks([_one([[(1, 1.0), (2, 1.0)]])])
    with pytest.raises(sa.SvdfError, match="exactly one private user entry.*none"):
        t.dataset_from_blocks([_one([[(NP + 3, 1.0)]])])
    with pytest.raises(sa.SvdfError, match="must belong to one user"):
        t.dataset_from_blocks([_one([[(1, 1.0), (NP + 3, 1.0)], [(NP + 3, 1.0), (2, 1.0)]])])
    with pytest.raises(sa.SvdfError, match="must belong to one user"):
        t.dataset_from_blocks([_one([[(1, 1.0), (NP + 3, 1.0)]], TAG_START), _one([[(2, 1.0), (NP + 3, 1.0)]], TAG_END)])
    with pytest.raises(sa.SvdfError, match="shared user id listed twice"):
        t.dataset_from_blocks([_one([[(1, 1.0), (NP + 3, 1.0), (NP + 3, 0.5)]])])
    shared = [_one([[(1, 1.0), (NP + 3, 1.0)]])]
    b = _trainer(conf, 0, MB + [("amd:contrib", "bf16")])
    with pytest.raises(sa.SvdfError, match="amd:contrib = fp32"):
        b.dataset_from_blocks(shared)
    w = _trainer(conf, 0, [("amd:shared_user_from", NP)])
    with pytest.raises(sa.SvdfError, match="svdf_dataset_window_from_blocks.*N-rank"):
        w.dataset_window_from_blocks(BlockArrays.from_blocks(shared))
    p = _trainer(conf, 0, [("amd:step", "minibatch")])   # without the key the message stays the one of today
    with pytest.raises(sa.SvdfError, match="exactly one user"):
        p.dataset_from_blocks(shared)
    g = sa.Trainer(1, 0)
    g.set_param("amd:gpus", "2")
    with pytest.raises(sa.SvdfError, match="one GPU only"):
        g.set_param("amd:shared_user_from", str(NP))
    for knob, what in (("window_shared_sub", "window_shared_sub"), ("window_item_sub", "window_item_sub")):   # the ordered sub-step lanes stay refused
        s = _trainer(conf, 0, MB, [(knob, 4)])
        with pytest.raises(sa.SvdfError, match=what + ".*not supported with user-group"):
            s.dataset_from_blocks(shared)
    # ... and so do the pair lane and side tables with a user-group trainer
    pr = _trainer(_conf(8, active=3), 3, MB, [("window_pair_sub", 12)])
    with pytest.raises(sa.SvdfError, match=r"window_pair_sub > 0 .* is not supported with user-group \(SVD\+\+\) trainers"):
        pr.dataset_from_pairs(np.array([1, 1, 2], np.uint32), np.array([3, 4, 5], np.uint32), np.array([6, 7, 8], np.uint32))


def test_side_tables_stay_refused_with_user_group_trainers(tmp_path):
    fu = str(tmp_path / "fu.txt")
    with open(fu, "w") as f:   # every user id has the shared id NP + 1 as its one child
        for _ in range(NP + NS):
            f.write("1 %d:1\n" % (NP + 1))
    t = _trainer(_conf(8) + [("feature_user", fu)], 0, MB)
    with pytest.raises(sa.SvdfError, match=r"side tables are not supported with user-group \(SVD\+\+\) trainers"):
        t.dataset_from_blocks([_one([[(1, 1.0), (NP + 3, 1.0)]])])


def test_the_buffer_file_route_equals_the_block_route(tmp_path):
    """svdf_dataset_from_buffer_file(.., 1) on a user-group buffer whose rows carry shared ids: the same windows and bits as svdf_dataset_from_blocks"""
    from svdfeature_amd import data as D
    conf = _conf(64)
    blocks = _blocks(21, max_shared=3, split_every=3)
    path = str(tmp_path / "shared.ug")
    D.write_ugroup_buffer(path, blocks)
    ba = BlockArrays.from_blocks(blocks)
    a, _ = _run(conf, ba)
    b = _trainer(conf, 0, MB + _window_key(ba))
    ds = b.dataset_from_buffer_file(path, user_group=True)
    assert ds.kind == 8 and ds.num_batches == 3
    for _ in range(2):
        b.train_dataset(ds)
    b.synchronize()
    _same(_views(a), _views(b))
    assert b.counter(33) + b.counter(34) == 6 and a.counter(34) == b.counter(34)
    p = _trainer(conf, 0, [("amd:step", "minibatch")] + _window_key(ba))   # without the key the file's rows are refused as today
    with pytest.raises(sa.SvdfError, match="exactly one user"):
        p.dataset_from_buffer_file(path, user_group=True)


def test_short_fuzz_run():
    import fuzz_block_shared
    assert fuzz_block_shared.run(iters=30, seed=7) == 0

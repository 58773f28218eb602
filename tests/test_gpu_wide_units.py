"""The window step of USER UNITS at wide factor rows, 256 < num_factor <= 1024: rows with global features or several user /
item entries, SVD++ blocks, `amd:shared_user_from` rows and feature_user / feature_item side tables on the one-GPU window sequence of
`amd:step = minibatch`, through k_wunit_walk / k_wunit_sum / k_wunit_score with a whole wave per unit, target or row (WideRow<2..4>: two, three or four
float4 per lane).  The semantics are those of the narrow widths, so the checkers are the ones of the narrow tests -- tests/multi_rank_utils.py,
tests/window_sim.py -- and every comparison is on uint32 views."""
import numpy as np
import pytest

import cases
import multi_rank_utils
import svdfeature_amd as sa
import window_sim as ws
from multi_rank_utils import simulate
from svdfeature_amd import BlockArrays, CSRData
from test_gpu_wunit import SVDPP_NAMES, _rows_with_globals
from test_window_blocks import SVDPP_EXTRA

pytestmark = pytest.mark.gpu
ROW_NAMES = ("W_item", "i_bias", "g_bias", "W_user", "u_bias")
MB = [("amd:step", "minibatch")]


@pytest.fixture(scope="module", autouse=True)
def _port():
    from oracle import oracle
    oracle.build()


def _trainer(conf, fmt=0, active=0, extra=(), knobs=()):
    t = sa.Trainer(fmt, active)
    t.seed(10)
    for k, v in list(conf) + list(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _same(t, o, names, what=None):
    for name in names:
        a, b = t.view(name), o.view(name)
        assert np.isfinite(a).all(), (name, what)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, what)


def _binary(labels):
    labels[:] = (labels > 3).astype(np.float32)
    assert set(np.unique(labels)) == {0.0, 1.0}


def _sequence(conf, data, windows, passes, fmt=0, active=0, extra=(), knobs=()):
    """the one-GPU window sequence of `windows` windows (amd:window in rows), trained `passes` times"""
    t = _trainer(conf, fmt, active, MB + [("amd:window", -(-data.num_row // windows))] + list(extra), knobs)
    ds = t.dataset_from_blocks(data) if fmt == 1 else t.dataset_from_csr(data)
    assert ds.kind == 8 and ds.num_batches == windows, (ds.kind, ds.num_batches)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    return t, ds


# ------------------------------------------------------------------------------------------------- 1. widths, csr rows
def _row_conf(k, nu=150, ni=40, ng=12, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_global=ng, wd_global="0.001") + list(extra)


@pytest.mark.parametrize("k,fixed", [(257, False), (260, False), (320, False), (512, False), (515, False), (768, False), (770, False), (1000, False),
                                     (1024, False), (320, True), (256, False), (64, False)])
def test_rows_with_globals_at_every_wide_width_equal_the_stale_sum_simulation(k, fixed):
    """two, three and four float4 per lane, full and ragged last slots, k % 4 in {0, 1, 2, 3}; ragged global sections, a second item entry and
    non-unit user values (rptr), and the fixed layout (estride) once.  k = 256 and 64: the narrow instantiations of the same kernels still equal
    the checker, which is what the parent commit's library gives."""
    d = _rows_with_globals(2000, 150, 40, 12, 3, k, fixed=fixed)
    conf = _row_conf(k)
    t, _ = _sequence(conf, d, 3, 2)
    _same(t, simulate(conf, d, None, None, 1, 3, 2, minibatch=True)[0].t, ROW_NAMES, k)


def _ragged_rows(k, seed, binary=False):
    """2 000 ragged rows: 0 .. 3 global entries, sometimes a second item entry, user values 1 / 0.5 (tests/test_gpu_wunit._rows_with_globals)"""
    d = _rows_with_globals(2000, 150, 40, 12, 3, seed, fixed=False)
    if binary:
        _binary(d.row_label)
    return d


SIGMOID = (("base_score", "0.5"),)
RANGES = (("up:wd", "0.1"), ("up:bound", "60"), ("up:wd", "0.002"), ("up:bound", "100000"), ("ip:wd", "0.05"), ("ip:bound", "15"), ("ip:wd", "0.004"),
          ("ip:bound", "100000"), ("num_regfree_global", "2"), ("gp:wd", "0.1"), ("gp:bound", "5"), ("gp:wd", "0.002"), ("gp:bound", "100"))


@pytest.mark.parametrize("k,active,extra", [(515, 1, SIGMOID), (515, 2, SIGMOID), (515, 5, SIGMOID), (515, 7, SIGMOID),
                                            (515, 0, (("reg_method", "1"),)), (1000, 0, (("reg_method", "2"), ("wd_user", "0.5"), ("wd_item", "0.5"))),
                                            (515, 0, (("reg_method", "3"),)), (515, 0, (("reg_global", "1"), ("num_regfree_global", "2"))),
                                            (515, 0, (("user_nonnegative", "1"),)), (515, 0, (("no_user_bias", "1"),)), (515, 0, RANGES),
                                            (1000, 0, (("reg_method", "2"), ("wd_user", "0.1"), ("wd_item", "0.1")))])
def test_links_and_regularisers_on_rows_with_globals_at_wide_widths(k, active, extra):
    """k_wunit_walk<64, false, false, WideRow<3 / 4>> beyond the linear link and L2: the sigmoid links (1, 2, 7) and the smooth hinge (5) on binary
    labels, L1 on every row (1) and on the user rows alone (3), the projection (2: group_dot over a wide row, at k = 1000), L1 on the global
    biases with two of them free, the nonnegative clamp, no user bias, split up: / ip: / gp: ranges.  Ragged rows, a second item entry, non-unit
    user values; 515 = 2 * 256 + 3.  Under the bound 0.5 no row is ever scaled (the squared norms stay near 0.1 at k = 1000: the dot is formed and
    must stay below the bound); the last case puts the bound at 0.1, inside the rows' norms: in the simulation 46 of the 150 user rows end on it."""
    d = _ragged_rows(k, 40 + active + len(extra), binary=active != 0)
    conf = _row_conf(k, extra=extra)
    t, _ = _sequence(conf, d, 3, 2, active=active)
    _same(t, simulate(conf, d, None, None, 1, 3, 2, active=active, minibatch=True)[0].t, ROW_NAMES, (k, active, extra))


def _simulate_rounds(conf, d, windows, passes):
    """multi_rank_utils.simulate for one rank with the reference's round protocol around every pass: set_round(p), the pass, finish_round"""
    from svdfeature_amd.multi_gpu import shard_csr_windows
    a = multi_rank_utils.OracleShard(multi_rank_utils.make_oracle(conf), minibatch=True)
    wins = a.make_windows(shard_csr_windows(d, 0, 1, windows))
    for p in range(passes):
        a.t.set_round(p)
        for w in wins:
            a.delta_begin()
            a.train(w)
            a.delta_set(a.delta_get().copy())
        a.t.finish_round()
    return a.t


def test_the_decayed_learning_rate_reaches_the_wide_walk_between_two_passes():
    """decay_learning_rate = 1, decay_rate = 0.5: set_round(1) after the first pass halves the rate on both sides (the window sequence honours it:
    Engine::set_round marks the kernel parameters dirty and the next pass reads them); without the set_round calls the model is another one"""
    k = 515
    d = _ragged_rows(k, 77)
    conf = _row_conf(k, extra=(("decay_learning_rate", "1"), ("decay_rate", "0.5")))
    t = _trainer(conf, 0, 0, MB + [("amd:window", -(-d.num_row // 3))])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and ds.num_batches == 3
    for p in range(2):
        t.set_round(p)
        t.train_dataset(ds)
        t.finish_round()
    t.synchronize()
    _same(t, _simulate_rounds(conf, d, 3, 2), ROW_NAMES)
    flat = simulate(conf, d, None, None, 1, 3, 2, minibatch=True)[0].t   # no set_round: the rate never decays
    assert not np.array_equal(flat.view("W_item"), t.view("W_item"))


# ------------------------------------------------------------------------------------------------- 1b. contribution counts at the sums' group edges
EDGE_K = 770
ROW_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 17)   # rows of the window that meet one item / one global id: around the in-place sums' groups of 4 slots
FB_COUNTS = (1, 3, 4, 5, 8, 9)              # segments of the window whose list names one feedback id: around the deferred sum's groups of 4 records


def _edge_rows():
    """56 rows in one window: item j is met by ROW_COUNTS[j] rows and global id j by ROW_COUNTS[j] rows (items 9 .. 11 and ids 9, 10 by none)"""
    rng = np.random.default_rng(3)
    items = rng.permutation(np.repeat(np.arange(len(ROW_COUNTS)), ROW_COUNTS))
    gids = rng.permutation(np.repeat(np.arange(len(ROW_COUNTS)), ROW_COUNTS))
    rows = [(float(rng.integers(1, 6)), [(int(g), float(rng.uniform(0.1, 1.0)))], [(int(rng.integers(0, 30)), float(rng.choice([1.0, 0.5])))], [(int(i), 1.0)])
            for i, g in zip(items, gids)]
    return CSRData.from_rows(rows)


@pytest.mark.parametrize("inplace", [1, 0])
@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
def test_item_and_global_rows_met_by_1_to_17_rows_of_one_window(contrib, inplace):
    """k_wunit_sum in place over WideRow<4> (770 = 3 * 256 + 2): rows with 1 (applied in place under wunit_inplace = 1), 2, 3, 4, 5, 7, 8, 9 and 17
    contributions, which the sum requests 4 slots at a time -- a short group, a full group, one over, two groups, four groups and one"""
    d = _edge_rows()
    ni, ng = 12, 11
    assert d.num_row == sum(ROW_COUNTS) and np.array_equal(d.row_ptr, np.arange(3 * d.num_row + 1))   # one global, one user, one item entry per row
    glob_col, item_col = d.feat_index.reshape(-1, 3)[:, 0], d.feat_index.reshape(-1, 3)[:, 2]
    assert tuple(np.bincount(item_col, minlength=ni)) == ROW_COUNTS + (0, 0, 0) and tuple(np.bincount(glob_col, minlength=ng)) == ROW_COUNTS + (0, 0)
    conf = _row_conf(EDGE_K, 30, ni, ng)
    t = _trainer(conf, 0, 0, MB + [("amd:window", d.num_row), ("amd:contrib", contrib)], [("wunit_inplace", inplace)])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and ds.num_batches == 1
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    multi_rank_utils.CONTRIB_BF16 = contrib == "bf16"
    try:
        sim = simulate(conf, d, None, None, 1, 1, 2, minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    _same(t, sim[0].t, ROW_NAMES, (contrib, inplace))


def _edge_blocks():
    """10 users in one window, the third as a START / MIDDLE / END span: feedback id j is in the lists of FB_COUNTS[j] segments (ids 6, 7 in none)"""
    from svdfeature_amd.data import PlusBlock, TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START
    rng = np.random.default_rng(4)
    blocks = []
    for b in range(10):
        fb = np.array([j for j, c in enumerate(FB_COUNTS) if (b - j) % 10 < c], np.uint32)
        val = np.full(len(fb), 1.0 / np.sqrt(max(len(fb), 1)), np.float32)
        rows = CSRData.from_rows([(float(rng.integers(1, 6)), [], [(b, 1.0)], [(int(rng.integers(0, 30)), 1.0)]) for _ in range(3 + b % 3)])
        if b == 2:
            e = np.zeros(0, np.uint32), np.zeros(0, np.float32)
            blocks += [PlusBlock(fb, val, rows.slice_rows(0, 1), TAG_START), PlusBlock(e[0], e[1], rows.slice_rows(1, rows.num_row - 1), TAG_MIDDLE),
                       PlusBlock(fb, val, rows.slice_rows(rows.num_row - 1, rows.num_row), TAG_END)]
        else:
            blocks.append(PlusBlock(fb, val, rows, TAG_DEFAULT))
    segments = [b for b in blocks if b.extend_tag in (TAG_DEFAULT, TAG_START)]
    return blocks, np.bincount(np.concatenate([b.index_ufeedback for b in segments]).astype(np.int64), minlength=8)


@pytest.mark.parametrize("defer", [1, 0])
@pytest.mark.parametrize("inplace", [1, 0])
@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
def test_feedback_rows_named_by_1_to_9_segments_of_one_window(contrib, inplace, defer):
    """the deferred feedback sum (wunit_defer_fb = 1: k_wunit_sum forms the rows' contributions from the segments' deltas, DB = 4 records at a time)
    and the same rows through slots (0) over WideRow<4>: feedback ids named by 1, 3, 4, 5, 8 and 9 segments"""
    blocks, counts = _edge_blocks()
    assert tuple(counts) == FB_COUNTS + (0, 0) and len(blocks) == 12
    ba = BlockArrays.from_blocks(blocks)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=10, num_item=30, num_factor=EDGE_K, num_ufeedback=8) + SVDPP_EXTRA
    t = _trainer(conf, 1, 0, MB + [("amd:window", ba.num_row), ("amd:contrib", contrib)], [("wunit_inplace", inplace), ("wunit_defer_fb", defer)])
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches == 1
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    multi_rank_utils.CONTRIB_BF16 = contrib == "bf16"
    try:
        sim = simulate(conf, ba, None, None, 1, 1, 2, fmt=1, minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    _same(t, sim[0].t, SVDPP_NAMES, (contrib, inplace, defer))


# ------------------------------------------------------------------------------------------------- 2. SVD++ blocks
def _block_conf(k, nu=200, ni=70, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_ufeedback=ni) + SVDPP_EXTRA + list(extra)


def _svdpp(seed, binary=False):
    return BlockArrays.from_blocks(cases.user_blocks(120, 200, 70, 70, seed, max_rows=6, max_fb=5, split_every=5, binary_label=binary))


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("k", [260, 320, 768, 1024, 256, 64])
def test_svdpp_blocks_at_wide_widths_equal_the_stale_sum_simulation(k, defer):
    """DEFAULT blocks and START / MIDDLE / END spans; the feedback rows' contributions written as rows by the walk (wunit_defer_fb = 0) and formed by
    k_wunit_sum from the segments' deltas (1)"""
    ba = _svdpp(k)
    conf = _block_conf(k)
    t, ds = _sequence(conf, ba, 3, 2, fmt=1, knobs=[("wunit_defer_fb", defer)])
    _same(t, simulate(conf, ba, None, None, 1, ds.num_batches, 2, fmt=1, minibatch=True)[0].t, SVDPP_NAMES, (k, defer))


@pytest.mark.parametrize("active,extra", [(2, (("base_score", "0.5"),)), (0, (("reg_method", "1"),)), (0, (("reg_method", "2"), ("wd_user", "0.5"), ("wd_item", "0.5"))),
                                          (0, (("no_user_bias", "1"),)), (0, (("user_nonnegative", "1"),)),
                                          (0, (("up:wd", "0.1"), ("up:bound", "100"), ("up:wd", "0.002"), ("up:bound", "100000"))),
                                          (0, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")))])
def test_svdpp_links_and_regularisers_at_a_wide_width(active, extra):
    """the sigmoid link with binary labels, L1, the projection (group_dot over a wide row), no user bias, the nonnegative clamp, split up: ranges, a
    feedback learning rate of its own"""
    ba = _svdpp(3 + active, binary=active == 2)
    conf = _block_conf(320, extra=extra)
    t, ds = _sequence(conf, ba, 3, 2, fmt=1, active=active)
    _same(t, simulate(conf, ba, None, None, 1, ds.num_batches, 2, fmt=1, active=active, minibatch=True)[0].t, SVDPP_NAMES, extra)


# ------------------------------------------------------------------------------------------------- 3. shared user ids on csr rows
@pytest.mark.parametrize("k,reg,extra", [(320, 0, ()), (1024, 2, ()), (515, 0, (("no_user_bias", "1"),))])
def test_shared_user_rows_at_wide_widths_equal_the_checker(k, reg, extra):
    """the configuration of tests/test_gpu_shared_user_window.py: 60 private users, 200 shared ids (two of them hot), 360 rows in windows of 90, three
    passes, the private entry first / middle / last"""
    import test_gpu_shared_user_window as su
    conf = su._conf(k, reg, extra)
    d = su._data(k + reg)
    t = _trainer(conf, 0, 0, MB + [("amd:window", 90), ("amd:shared_user_from", su.NP)])
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and ds.num_batches == 4
    for _ in range(3):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.simulate_rows(ws.make_oracle(conf), d, su.NP, 4, 3, user_bias=dict(extra).get("no_user_bias") != "1")
    _same(t, o, su.VIEWS, k)


# ------------------------------------------------------------------------------------------------- 4. side tables
def test_side_tables_at_a_wide_width_equal_the_checker(tmp_path):
    """the "both" configuration of tests/test_gpu_side_table_window.py: feature_user children as shared user rows, feature_item children behind item
    entries with values != 1"""
    import test_gpu_side_table_window as st
    k = 320
    keys, tu, ti = st._tables(tmp_path, k, "both")
    conf = st._conf(k) + keys
    d = st._data(k, tu, ti)
    t = _trainer(conf, 0, 0, MB + [("amd:window", 90), ("amd:shared_user_from", st.NP)])
    ds = t.dataset_from_csr(d)
    W = ds.num_batches
    assert ds.kind == 8 and W == (d.num_row + 89) // 90 and d.num_row > 200
    for _ in range(2):
        t.train_dataset(ds)
    t.synchronize()
    _same(t, ws.simulate_rows(ws.make_oracle(conf), d, st.NP, W, 2, fu=tu, fi=ti), st.VIEWS)


# ------------------------------------------------------------------------------------------------- 5. blocks with shared ids
@pytest.mark.parametrize("fast", [None, 3])
@pytest.mark.parametrize("k,long_unit", [(320, False), (1024, False), (320, True)])
def test_blocks_with_shared_ids_at_wide_widths_equal_the_checker(k, long_unit, fast):
    """75 blocks with 1 .. 4 shared ids per user and non-unit values; the long-unit case: a unit of 150 rows, feedback lists of 0, 1 and 70 entries and a
    last one-row block whose shared id is applied in place.  Every window takes the general walk (counter 34), under wunit_fast = 3 too: the wave
    form stops at 256 factors (counter 33 stays 0)."""
    import test_gpu_block_shared_window as bs
    if long_unit:
        nf = 80
        conf = bs._conf(k, nf=nf)
        blocks = bs._blocks(k + 1, n=45, num_fb=nf, min_shared=1, max_shared=4, uvals=True, fb_sizes=(0, 1, 70, 3), long_unit=150, single=True)
    else:
        conf = bs._conf(k)
        blocks = bs._blocks(k, n=75, min_shared=1, max_shared=4, uvals=True)
    ba = BlockArrays.from_blocks(blocks)
    t, _ = bs._run(conf, ba, knobs=[("wunit_fast", fast)] if fast is not None else [])
    assert (t.counter(33), t.counter(34)) == (0, 6)
    o = ws.make_oracle(conf, user_group=True)
    ws.simulate_blocks(o, ba, bs.NP, 3, 2)
    bs._same(bs._views(t), {name: o.view(name) for name in bs.VIEWS})
    for name in ("W_user", "W_item", "W_ufeedback"):
        assert np.isfinite(t.view(name)).all(), name


# ------------------------------------------------------------------------------------------------- 6. bf16 slots
@pytest.mark.parametrize("shape,k", [("blocks", 320), ("rows", 512), ("blocks", 770), ("rows", 1023), ("blocks", 1024), ("rows", 515)])
def test_bf16_contribution_rows_at_wide_widths_equal_the_simulation_with_the_same_rounding(shape, k):
    """contrib_io<64, WideRow<2 / 3 / 4>> and the bf16 branch of the deferred feedback sum; 770, 1023 and 515 end in a ragged float4 (k % 4 = 2, 3, 3)"""
    if shape == "blocks":
        data = BlockArrays.from_blocks(cases.user_blocks(130, 200, 80, 80, seed=k, max_rows=12, max_fb=8, split_every=5))
        conf, fmt, names = _block_conf(k, 200, 80), 1, SVDPP_NAMES
    else:
        data = _rows_with_globals(3000, 300, 100, 30, 4, seed=k)
        conf, fmt, names = _row_conf(k, 300, 100, 30), 0, ROW_NAMES
    t, ds = _sequence(conf, data, 3, 2, fmt=fmt, extra=[("amd:contrib", "bf16")])
    multi_rank_utils.CONTRIB_BF16 = True
    try:
        sim = simulate(conf, data, None, None, 1, ds.num_batches, 2, fmt=fmt, minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    _same(t, sim[0].t, names)
    plain, _ = _sequence(conf, data, 3, 2, fmt=fmt)
    assert not np.array_equal(plain.view("W_item"), t.view("W_item"))   # the rounding took effect


# ------------------------------------------------------------------------------------------------- 7. in-place single applies
def _single_applies(shape, contrib, k):
    """the four knob combinations and the simulation; above 320 the blocks' catalogue is 1 400 items, which keeps the two item-side matrices near
    11 MB at about 350 rows per window"""
    windows = 4
    if shape == "blocks":
        nu, ni = 150, 2000 if k == 320 else 1400
        data = BlockArrays.from_blocks(cases.user_blocks(140, nu, ni, ni, seed=k, max_rows=20, max_fb=16, split_every=6))
        conf, fmt, names = _block_conf(k, nu, ni), 1, SVDPP_NAMES
    else:
        nu, ni, ng = 400, 3000, 30
        data = _rows_with_globals(2400, nu, ni, ng, 4, seed=k, fixed=False)
        conf, fmt, names = _row_conf(k, nu, ni, ng), 0, ROW_NAMES
    got = []
    for inplace, defer in ((1, 1), (0, 1), (1, 0), (0, 0)):
        t, ds = _sequence(conf, data, windows, 2, fmt=fmt, extra=[("amd:contrib", contrib)], knobs=(("wunit_inplace", inplace), ("wunit_defer_fb", defer)))
        got.append({name: t.view(name).copy() for name in names})
    multi_rank_utils.CONTRIB_BF16 = contrib == "bf16"
    try:
        sim = simulate(conf, data, None, None, 1, ds.num_batches, 2, fmt=fmt, minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    for name in names:
        for other in got[1:]:
            assert np.array_equal(got[0][name].view(np.uint32), other[name].view(np.uint32)), name
        assert np.array_equal(got[0][name].view(np.uint32), sim[0].t.view(name).view(np.uint32)), name


@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["blocks", "rows"])
def test_single_contributions_are_applied_in_place_with_the_same_bits_at_a_wide_width(shape, contrib):
    """many more items than rows per window, so most contributions are single (no slot: apply_single on a wide row): the default == every
    contribution through a slot (wunit_inplace = 0) == feedback contributions written as rows by the walk (wunit_defer_fb = 0) == the simulation"""
    _single_applies(shape, contrib, 320)


@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["blocks", "rows"])
@pytest.mark.parametrize("k", [700, 1022])
def test_single_contributions_are_applied_in_place_with_three_and_four_float4_per_lane(k, shape, contrib):
    """the same equalities over WideRow<3> (700) and WideRow<4> with a ragged last float4 (1022, k % 4 = 2)"""
    _single_applies(shape, contrib, k)


# ------------------------------------------------------------------------------------------------- 8. scoring
def _views_of(t, names):
    return {name: t.view(name).copy() for name in names if t.view(name) is not None}


def _check_scores(t, ds, want, labels, names):
    """predict_dataset == want bit for bit in file order, the evaluator against those predictions, the model untouched"""
    before = _views_of(t, names)
    got = t.predict_dataset(ds)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ss, cnt = t.eval_dataset(ds)
    assert cnt == len(want)
    diff = (got - np.asarray(labels, np.float32)).astype(np.float64)
    assert abs(ss - float(np.sum(diff * diff))) <= 1e-9 * ss
    t.synchronize()
    after = _views_of(t, names)
    for name in before:
        assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), name
    return got


def test_scoring_a_wide_csr_sequence_with_shared_entries_and_children(tmp_path):
    import test_gpu_window_scoring as ws
    k = 320
    keys, extra, d = ws._csr_case("d", tmp_path, seed=k)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=ws.NP_ + ws.NS_, num_item=ws.NT_ + ws.NA_, num_global=ws.NG_, num_factor=k, wd_global="0.002",
                           learning_rate="0.01") + keys
    t = _trainer(conf, 0, 0, MB + [("amd:window", 170)] + extra)
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and 3 <= ds.num_batches <= 4
    before = _check_scores(t, ds, t.predict_batch(d), d.row_label, ROW_NAMES)
    for _ in range(2):
        t.train_dataset(ds)
    after = _check_scores(t, ds, t.predict_batch(d), d.row_label, ROW_NAMES)
    assert not np.array_equal(before, after)


@pytest.mark.parametrize("defer", [0, 1])
def test_scoring_a_wide_block_sequence(defer):
    import test_gpu_window_scoring as ws
    k = 512
    nu, ni, blocks = ws._svdpp_blocks(seed=k + defer)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_ufeedback=ni, wd_ufeedback="0.004", ufeedback_init_sigma="0.01")
    ba = BlockArrays.from_blocks(blocks)
    t = _trainer(conf, 1, 0, MB + [("amd:window", 150)], [("wunit_defer_fb", defer)])
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches >= 3
    score = lambda: np.concatenate([t.predict_block(b) for b in blocks])
    before = _check_scores(t, ds, score(), ba.row_label, SVDPP_NAMES)
    for _ in range(2):
        t.train_dataset(ds)
    after = _check_scores(t, ds, score(), ba.row_label, SVDPP_NAMES)
    assert not np.array_equal(before, after)


@pytest.mark.parametrize("variant,k,active,extra", [("a", 768, 0, ()), ("b", 515, 0, ()), ("c", 1023, 0, ()), ("d", 1024, 0, ()),
                                                    ("b", 900, 2, (("base_score", "0.5"), ("no_user_bias", "1")))])
def test_scoring_wide_csr_sequences_of_every_layout_with_three_and_four_float4_per_lane(tmp_path, variant, k, active, extra):
    """k_wunit_score<false, WideRow<3 / 4>> on the four csr layouts of tests/test_gpu_window_scoring.py: the fixed layout (estride) at 768, ragged rows
    with two item entries and non-unit values (rptr) at 515 (k % 4 = 3), shared user entries at 1023 (k % 4 = 3), both side tables at 1024; the
    sigmoid link on binary labels without a user bias at 900.  Scored before and after two passes against predict_batch of the same trainer."""
    import test_gpu_window_scoring as ws
    keys, more, d = ws._csr_case(variant, tmp_path, seed=k)
    if active:
        _binary(d.row_label)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=ws.NP_ + ws.NS_, num_item=ws.NT_ + ws.NA_, num_global=ws.NG_, num_factor=k, wd_global="0.002",
                           learning_rate="0.01") + keys + list(extra)
    t = _trainer(conf, 0, active, MB + [("amd:window", 170)] + more)
    ds = t.dataset_from_csr(d)
    assert ds.kind == 8 and 3 <= ds.num_batches <= 4
    before = _check_scores(t, ds, t.predict_batch(d), d.row_label, ROW_NAMES)
    for _ in range(2):
        t.train_dataset(ds)
    after = _check_scores(t, ds, t.predict_batch(d), d.row_label, ROW_NAMES)
    assert not np.array_equal(before, after)


@pytest.mark.parametrize("k,defer,active,extra", [(700, 0, 0, ()), (700, 1, 0, ()), (1000, 0, 0, ()), (1000, 1, 0, ()),
                                                  (770, 1, 2, (("base_score", "0.5"), ("no_user_bias", "1")))])
def test_scoring_wide_block_sequences_with_three_and_four_float4_per_lane(k, defer, active, extra):
    """k_wunit_score_prepare and k_wunit_score<true, WideRow<3 / 4>>: START / MIDDLE / END spans, users without feedback and the feedback list of 70
    entries (more than one 64-record block), against predict_block of the same trainer; the sigmoid link without a user bias at 770 (k % 4 = 2)"""
    import test_gpu_window_scoring as ws
    nu, ni, blocks = ws._svdpp_blocks(seed=k + defer)
    assert any(b.num_ufeedback > 64 for b in blocks) and any(b.num_ufeedback == 0 for b in blocks)
    if active:
        for b in blocks:
            b.data.row_label[:] = (b.data.row_label > 3).astype(np.float32)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_ufeedback=ni, wd_ufeedback="0.004",
                           ufeedback_init_sigma="0.01") + list(extra)
    ba = BlockArrays.from_blocks(blocks)
    assert not active or set(np.unique(ba.row_label)) == {0.0, 1.0}
    t = _trainer(conf, 1, active, MB + [("amd:window", 150)], [("wunit_defer_fb", defer)])
    ds = t.dataset_from_blocks(ba)
    assert ds.kind == 8 and ds.num_batches >= 3
    score = lambda: np.concatenate([t.predict_block(b) for b in blocks])
    before = _check_scores(t, ds, score(), ba.row_label, SVDPP_NAMES)
    for _ in range(2):
        t.train_dataset(ds)
    after = _check_scores(t, ds, score(), ba.row_label, SVDPP_NAMES)
    assert not np.array_equal(before, after)


# ------------------------------------------------------------------------------------------------- 9. routes that stay
def test_sub_step_knobs_are_refused_at_a_wide_width_with_their_names():
    import test_gpu_block_shared_window as bs
    import test_gpu_shared_user_window as su
    d = su._data(1, n=40)
    for knob in ("window_shared_sub", "window_item_sub"):
        t = _trainer(su._conf(320), 0, 0, MB + [("amd:shared_user_from", su.NP)], [(knob, 4)])
        with pytest.raises(sa.SvdfError, match=knob + r" > 0 .* needs num_factor <= 256"):
            t.dataset_from_csr(d)
    ba = BlockArrays.from_blocks(bs._blocks(1, n=10, min_shared=1, max_shared=2))
    t = _trainer(bs._conf(320), 1, 0, bs.MB, [("window_block_sub", 4)])
    with pytest.raises(sa.SvdfError, match=r"window_block_sub > 0 .* needs num_factor <= 256"):
        t.dataset_from_blocks(ba)
    narrow = _trainer(su._conf(64), 0, 0, MB + [("amd:shared_user_from", su.NP)], [("window_shared_sub", 4)])
    assert narrow.dataset_from_csr(d).kind == 8   # the narrow width keeps the lane


def test_auto_keeps_wide_user_units_on_the_exact_levels():
    d = _rows_with_globals(20000, 300, 200, 8, 3, seed=1, fixed=True)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=300, num_item=200, num_global=8, num_factor=320, wd_global=0.001)
    t = _trainer(conf, 0, 0, [("amd:step", "auto")])
    ds = t.dataset_from_csr(d)
    assert ds.kind != 8
    m = _trainer(conf, 0, 0, MB)
    assert m.dataset_from_csr(d).kind == 8   # asked for by name, the same rows take the window step


def test_the_verbose_line_names_the_wide_general_walk(monkeypatch, capfd):
    monkeypatch.setenv("SVDF_VERBOSE", "1")
    monkeypatch.delenv("SVDF_QUIET", raising=False)
    d = _rows_with_globals(300, 150, 40, 12, 3, 1, fixed=False)
    for k, named in ((320, True), (64, False)):
        capfd.readouterr()
        assert _trainer(_row_conf(k), 0, 0, MB).dataset_from_csr(d).kind == 8
        assert ("wide general walk" in capfd.readouterr().err) == named


# ------------------------------------------------------------------------------------------------- 10. the accuracy contract
def test_the_window_step_keeps_the_accuracy_contract_on_rows_with_globals_at_a_wide_width():
    """60 000 planted ratings, each with 2 of 50 global ids (values U(0.1, 1)), k = 320, windows of 1 500 rows (40 windows), three passes: held-out
    RMSE on 6 000 further rows within 1e-4 of the exact pass of the same build -- the contract of every window step.  The checkers alone on the CPU
    give exact 0.732444 and window 0.732482 on this input, a difference of 3.8e-5 (1.1e-4 at 20 windows); both engine paths equal their checkers
    bit for bit, so the figures printed here are those."""
    nu, ni, ng, n, k = 5000, 1000, 50, 60000, 320
    u, i, r = cases.planted_triples(n + 6000, nu, ni, seed=21)
    rng = np.random.default_rng(5)
    N = n + 6000
    gid, gval = np.empty((N, 2), np.uint32), np.empty((N, 2), np.float32)
    for row in range(N):   # row by row: 2 distinct ids in ascending order, then their values (the draw order of test_gpu_wunit._rows_with_globals)
        gid[row] = sorted(rng.choice(ng, size=2, replace=False))
        gval[row] = [rng.uniform(0.1, 1.0) for _ in range(2)]
    idx = np.concatenate([gid, u[:, None].astype(np.uint32), i[:, None].astype(np.uint32)], axis=1)
    val = np.concatenate([gval, np.ones((N, 2), np.float32)], axis=1)
    ptr = np.empty(3 * N + 1, np.int64)
    base = 4 * np.arange(N, dtype=np.int64)
    ptr[0:3 * N:3], ptr[1:3 * N:3], ptr[2:3 * N:3], ptr[3 * N] = base, base + 2, base + 3, 4 * N
    full = CSRData(r, ptr, idx.ravel(), val.ravel())
    train, test, tl = full.slice_rows(0, n), full.slice_rows(n, N), r[n:]
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=ng, num_factor=k, wd_global="0.001")
    out = []
    for extra in ([], MB + [("amd:window", 1500)]):
        t = _trainer(conf, 0, 0, extra)
        ds = t.dataset_from_csr(train)
        for _ in range(3):
            t.train_dataset(ds)
        p = t.predict_batch(test)
        assert np.isfinite(p).all()
        out.append((float(np.sqrt(np.mean((p.astype(np.float64) - tl) ** 2))), ds.num_batches, ds.kind))
    print("held-out RMSE: exact %.6f window %.6f difference %.3g (%d windows)" % (out[0][0], out[1][0], out[1][0] - out[0][0], out[1][1]))
    assert out[0][2] != 8 and out[1][2] == 8 and out[1][1] == 40
    assert abs(out[1][0] - out[0][0]) <= 1e-4, out


def svdpp_contract_input(nu=4000, ni=800, n=60000, held=6000, k=320):
    """planted ratings grouped into one SVD++ block per user, the users in a random order; a user's feedback list is the set of items of its training
    rows at value n^-1/2; the held-out rows are grouped the same way and carry the training lists.  (conf, training blocks, test blocks, test labels)"""
    from svdfeature_amd.data import PlusBlock, TAG_DEFAULT
    u, i, r = cases.planted_triples(n + held, nu, ni, seed=23)
    order = np.argsort(u[:n], kind="stable")
    lo = np.searchsorted(u[:n][order], np.arange(nu + 1))
    horder = n + np.argsort(u[n:], kind="stable")
    hlo = np.searchsorted(u[horder], np.arange(nu + 1))
    train, test, labels = [], [], []
    for uid in np.random.default_rng(9).permutation(nu):
        m, h = order[lo[uid]:lo[uid + 1]], horder[hlo[uid]:hlo[uid + 1]]
        fb = np.unique(i[m]).astype(np.uint32)
        val = np.full(len(fb), 1.0 / np.sqrt(max(len(fb), 1)), np.float32)
        if len(m):
            train.append(PlusBlock(fb, val, CSRData.from_triples(u[m], i[m], r[m]), TAG_DEFAULT))
        if len(h):
            test.append(PlusBlock(fb, val, CSRData.from_triples(u[h], i[h], r[h]), TAG_DEFAULT))
            labels.append(r[h])
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, num_ufeedback=ni) + SVDPP_EXTRA
    return conf, train, test, np.concatenate(labels).astype(np.float64)


def test_the_window_step_keeps_the_accuracy_contract_on_svdpp_blocks_at_a_wide_width():
    """60 000 planted ratings of 4 000 users on 800 items as one SVD++ block per user (feedback list: the user's training items at n^-1/2), k = 320,
    windows of 1 500 rows (40 windows, cut at block positions), three passes: held-out RMSE on 6 000 further rows, scored with predict_block under
    the training lists, within 1e-4 of the exact pass of the same build.  The checkers alone on the CPU (oracle update_block against
    simulate(fmt = 1, minibatch)) give exact 0.723293 and window 0.723345 on this input, a difference of 5.2e-5 (8.3e-5 at 20 windows, 1.6e-5 at
    60); both engine paths equal their checkers bit for bit, so the figures printed here are those."""
    conf, train, test, tl = svdpp_contract_input()
    ba = BlockArrays.from_blocks(train)
    assert ba.num_row == 60000 and len(tl) == 6000
    out = []
    for extra in ([], MB + [("amd:window", 1500)]):
        t = _trainer(conf, 1, 0, extra)
        ds = t.dataset_from_blocks(ba)
        for _ in range(3):
            t.train_dataset(ds)
        p = np.concatenate([t.predict_block(b) for b in test])
        assert np.isfinite(p).all()
        out.append((float(np.sqrt(np.mean((p.astype(np.float64) - tl) ** 2))), ds.num_batches, ds.kind))
    print("held-out RMSE: exact %.6f window %.6f difference %.3g (%d windows)" % (out[0][0], out[1][0], out[1][0] - out[0][0], out[1][1]))
    assert out[0][2] != 8 and out[1][2] == 8 and out[1][1] == 40
    assert abs(out[1][0] - out[0][0]) <= 1e-4, out

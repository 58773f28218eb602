"""The window step of USER UNITS at wide factor rows, 256 < num_factor <= 1024: rows with global features or several user /
item entries, SVD++ blocks, `amd:shared_user_from` rows and feature_user / feature_item side tables on the one-GPU window sequence of
`amd:step = minibatch`, through k_wunit_walk / k_wunit_sum / k_wunit_score with a whole wave per unit, target or row (WideRow<2..4>: two, three or four
float4 per lane).  The semantics are those of the narrow widths, so the checkers are the ones of the narrow tests -- tests/multi_rank_utils.py,
shared_user_sim.py, side_table_sim.py, block_shared_sim.py -- and every comparison is on uint32 views."""
import numpy as np
import pytest

import block_shared_sim
import cases
import multi_rank_utils
import shared_user_sim
import side_table_sim as sts
import svdfeature_amd as sa
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
    o = shared_user_sim.simulate(shared_user_sim.make_oracle(conf), d, su.NP, 4, 3, user_bias=dict(extra).get("no_user_bias") != "1")
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
    _same(t, sts.simulate(shared_user_sim.make_oracle(conf), d, st.NP, W, 2, tu, ti), st.VIEWS)


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
    o = block_shared_sim.simulate(block_shared_sim.make_oracle(conf), ba, bs.NP, 3, 2)
    bs._same(bs._views(t), {name: o.view(name) for name in bs.VIEWS})
    for name in ("W_user", "W_item", "W_ufeedback"):
        assert np.isfinite(t.view(name)).all(), name


# ------------------------------------------------------------------------------------------------- 6. bf16 slots
@pytest.mark.parametrize("shape,k", [("blocks", 320), ("rows", 512)])
def test_bf16_contribution_rows_at_wide_widths_equal_the_simulation_with_the_same_rounding(shape, k):
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
@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ["blocks", "rows"])
def test_single_contributions_are_applied_in_place_with_the_same_bits_at_a_wide_width(shape, contrib):
    """many more items than rows per window, so most contributions are single (no slot: apply_single on a wide row): the default == every
    contribution through a slot (wunit_inplace = 0) == feedback contributions written as rows by the walk (wunit_defer_fb = 0) == the simulation"""
    k, windows = 320, 4
    if shape == "blocks":
        nu, ni = 150, 2000
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

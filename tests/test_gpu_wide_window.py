"""The window step at wide factor rows, 256 < num_factor <= 1024: plain ratings and rank pairs through svdf_k_window.hip with a
whole wave per row (WideRow<2..4>: two, three or four float4 per lane).  The semantics are those of the narrow widths, so the checkers are the same:
the stale-sum simulation of tests/multi_rank_utils.py (oracle/svdf_oracle.c: svdo_update_csr_batch_stale, bf16 slots through svdo_set_stale_rounding)
and svdo_update_window_substeps for the lane of ordered sub-steps.  Every comparison is on the uint32 views of W_item, i_bias, W_user, u_bias unless a
test says otherwise."""
import numpy as np
import pytest

import cases
import multi_rank_utils
import svdfeature_amd as sa
from multi_rank_utils import simulate, simulate_parts
from svdfeature_amd import CSRData
from svdfeature_amd.multi_gpu import Pairs
from test_gpu_window import _check as _check_ranks
from test_gpu_window import _run_ranks

pytestmark = pytest.mark.gpu
NAMES = ("W_item", "i_bias", "W_user", "u_bias")
MB = [("amd:step", "minibatch")]


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


def _same_model(t, o, names=NAMES, what=None):
    for name in names:
        a, b = t.view(name), o.view(name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, what)


def _sequence(conf, u, i, r, windows, passes, active=0, extra=(), knobs=(("window_hot_sub", 0),)):
    """the one-GPU window sequence of `windows` equal windows, trained `passes` times"""
    n = len(r)
    t = _trainer(conf, active, MB + [("amd:window", -(-n // windows))] + list(extra), knobs)
    ds = t.dataset_from_triples(u, i, r)
    assert ds.kind == 8 and ds.num_batches == windows
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    return t


# ------------------------------------------------------------------------------------------------- 1. widths
def _width_data():
    nu, ni, n = 600, 90, 6000
    u, i, r = cases.planted_triples(n, nu, ni, seed=21)
    u[:600] %= 7     # a few heavy users: long sequential walks
    i[i == 5] = 6    # an item nobody rates
    return nu, ni, u, i, r


@pytest.mark.parametrize("k", [257, 260, 320, 512, 515, 768, 770, 1000, 1024])
def test_every_wide_width_equals_the_stale_sum_simulation(k):
    """two, three and four float4 per lane, full and ragged last slots, k % 4 in {0, 1, 2, 3}"""
    nu, ni, u, i, r = _width_data()
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    t = _sequence(conf, u, i, r, 3, 2)
    _same_model(t, simulate(conf, u, i, r, 1, 3, 2, minibatch=True)[0].t)


@pytest.mark.parametrize("shape", ["one_user", "one_item", "one_instance", "every_user_once"])
def test_degenerate_window_shapes_at_a_wide_width(shape):
    nu, ni, n, k = 600, 90, 6000, 320
    u, i, r = cases.planted_triples(n, nu, ni, seed=21)
    if shape == "one_user":
        u[:] = 7
    elif shape == "one_item":
        i[:] = 11
    elif shape == "one_instance":
        u, i, r = u[:1], i[:1], r[:1]
    else:
        u, i, r = np.arange(nu, dtype=np.uint32), i[:nu], r[:nu]
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    windows = 1 if len(r) < 10 else 3
    t = _sequence(conf, u, i, r, windows, 2)
    _same_model(t, simulate(conf, u, i, r, 1, windows, 2, minibatch=True)[0].t)


# ------------------------------------------------------------------------------------------------- 2. links and regularisers
@pytest.mark.parametrize("active,extra", [(2, (("base_score", "0.5"),)), (0, (("reg_method", "1"),)), (0, (("reg_method", "2"), ("wd_user", "0.5"), ("wd_item", "0.5"))),
                                          (0, (("no_user_bias", "1"),)), (0, (("user_nonnegative", "1"),)), (0, (("up:wd", "0.1"), ("up:bound", "100"), ("up:wd", "0.002"), ("up:bound", "100000")))])
def test_other_links_and_regularisers_at_a_wide_width(active, extra):
    nu, ni, n = 400, 150, 8000
    u, i, r = cases.planted_triples(n, nu, ni, seed=3)
    if active == 2:
        r = (r > 3).astype(np.float32)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=320) + list(extra)
    ranks = _run_ranks(conf, u, i, r, 2, 3, 2, active=active)
    _check_ranks(ranks, simulate(conf, u, i, r, 2, 3, 2, active=active, minibatch=True))


# ------------------------------------------------------------------------------------------------- 3. long and sparse lists, both slot formats, the wire
@pytest.mark.parametrize("k,ni,contrib", [(320, 9, "fp32"), (320, 9, "bf16"), (1024, 9, "fp32"), (1024, 9, "bf16"),
                                          (320, 30000, "fp32"), (320, 30000, "bf16"), (1024, 30000, "fp32"), (1024, 30000, "bf16")])
def test_long_and_sparse_lists_in_both_slot_formats(k, ni, contrib):
    """ni = 9: every list has hundreds of slots (a wave adds them four at a time); ni = 30 000: 6 000 ratings over 30 000 items with two hot ones
    (2 000 / 850 slots per window) -- the sparse form, a lane per item's list bounds.  Wire buffers of two simulated ranks and the in-place sums of
    the one-GPU sequence."""
    nu, n, windows = 2000, 24000, 4
    u, i, r = cases.planted_triples(n, nu, ni, seed=k + ni)
    if ni >= 2000:
        i[::3] = 7
        i[1::7] = 11
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, learning_rate=0.0005)
    multi_rank_utils.CONTRIB_BF16 = contrib == "bf16"
    try:
        sim2 = simulate(conf, u, i, r, 2, windows, 2, minibatch=True)
        sim1 = simulate(conf, u, i, r, 1, windows, 2, minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    conf_c = conf + [("amd:contrib", contrib)]
    _check_ranks(_run_ranks(conf_c, u, i, r, 2, windows, 2), sim2)
    t = _sequence(conf_c, u, i, r, windows, 2)
    _same_model(t, sim1[0].t)


def test_fp16_wire_stays_close_and_item_range_pieces_are_exact_at_wide_widths():
    nu, ni, n = 1200, 400, 20000
    u, i, r = cases.planted_triples(n, nu, ni, seed=21)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=512)
    full = _run_ranks(conf, u, i, r, 2, 4, 2)
    half = _run_ranks(conf, u, i, r, 2, 4, 2, half=True)
    a, b = full[0].t.view("W_item"), half[0].t.view("W_item")
    assert np.abs(a - b).max() <= 1e-3 * np.abs(a).max() and not np.array_equal(a, b)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=320)
    pieces = _run_ranks(conf, u, i, r, 2, 4, 2, parts=2, num_item=ni)
    _check_ranks(pieces, simulate_parts(conf, u, i, r, 2, 4, 2, 2, ni, minibatch=True))


@pytest.mark.parametrize("k", [320, 1024])
@pytest.mark.parametrize("ni", [9, 30000])
def test_fp16_wire_buffer_is_the_fp32_one_rounded_to_nearest_even_at_wide_widths(k, ni):
    """k_window_items_wide's fp16 writer: ni = 9, a wave per item (span = 1); ni = 30 000, 6 000 ratings: the sparse form (span = 64), items without
    slots written as zeros"""
    from test_gpu_window import _fp16_wire_is_the_rounded_fp32_wire
    nu, n = 2000, 6000
    u, i, r = cases.planted_triples(n, nu, ni, seed=k + ni)
    _fp16_wire_is_the_rounded_fp32_wire(cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k), u, i, r)


def test_stratified_schedule_with_in_place_sums_into_item_blocks_at_a_wide_width():
    """svdf_window_delta_apply_local on an item block [lo, hi) with lo > 0, svdf_item_block_get / _set and the trainer class over them: the
    schedule test of tests/test_gpu_window.py at k = 320, two ranks"""
    import test_gpu_window as tw
    tw.test_stratified_schedule_on_simulated_ranks_equals_the_simulation(320, 2, 1, 701)


# ------------------------------------------------------------------------------------------------- 4. rank pairs
@pytest.mark.parametrize("k", [384, 1000])
def test_rank_pairs_sequence_and_simulated_ranks(k):
    import torch
    from svdfeature_amd.multi_gpu import HipShard, shard_pair_windows
    nu, ni, n, windows, passes = 400, 120, 8000, 4, 2
    u, p, q = cases.planted_pairs(n, nu, ni, seed=k)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, learning_rate=0.05, ui_init_sigma=0.1)
    names = ("W_item", "i_bias", "W_user")
    # the one-GPU sequence
    t = _trainer(conf, 3, MB + [("amd:window", n // windows)])
    ds = t.dataset_from_pairs(u, p, q)
    assert ds.kind == 8 and ds.num_batches == windows
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    _same_model(t, simulate(conf, Pairs(u, p, q), None, None, 1, windows, passes, active=3, minibatch=True)[0].t, names)
    # two simulated ranks of stand-alone windows
    dev = torch.device("cuda", 0)
    ranks = []
    for rk in range(2):
        ad = HipShard(_trainer(conf, 3), torch, dev, minibatch=True)
        ad.set_wire_half(False)
        ranks.append((ad, ad.make_windows(shard_pair_windows(u, p, q, rk, 2, windows))))
    assert ranks[0][1][0].kind == 5
    for _ in range(passes):
        for w in range(windows):
            ds_ = []
            for ad, wins in ranks:
                ad.train(wins[w])
                d = ad.delta_get()
                ad.stream.synchronize()
                ds_.append(d.clone())
            total = ds_[0] + ds_[1]
            torch.cuda.synchronize()
            for ad, _ in ranks:
                ad.delta_set(total)
    sim = simulate(conf, Pairs(u, p, q), None, None, 2, windows, passes, active=3, minibatch=True)
    for (ad, _), s in zip(ranks, sim):
        ad.t.synchronize()
        _same_model(ad.t, s.t, names)
    with pytest.raises(sa.SvdfError, match="must differ"):
        ranks[0][0].t.dataset_window_from_pairs(u[:3], p[:3], p[:3])


# ------------------------------------------------------------------------------------------------- 5. ordered sub-steps for hot items
def _substep_oracle(conf, active, u, i, r, windows, sub, passes):
    from oracle import oracle
    oracle.build()
    o = oracle.OracleTrainer("port", 0, active)
    o.seed(10)
    for k, v in conf:
        o.set_param(k, v)
    o.init_model()
    o.init_trainer()
    n = len(r)
    ws = [CSRData.from_triples(u[n * w // windows:n * (w + 1) // windows], i[n * w // windows:n * (w + 1) // windows], r[n * w // windows:n * (w + 1) // windows])
          for w in range(windows)]
    for _ in range(passes):
        for d in ws:
            o.update_window_substeps(d, sub)
    return o


@pytest.mark.parametrize("k,active,extra,sub", [(260, 0, (), 16), (512, 0, (), 16), (1024, 0, (), 16), (768, 0, (), 100),
                                              (320, 2, (("base_score", "0.5"),), 16), (320, 0, (("reg_method", "1"),), 16)])
def test_hot_items_move_in_ordered_sub_steps_at_wide_widths(k, active, extra, sub):
    nu, ni, n, passes = 3000, 150, 60000, 2
    u, i, r = cases.planted_triples(n, nu, ni, seed=k + sub, zipf=True)
    if active == 2:
        r = (r > 3).astype(np.float32)
    cnt = np.bincount(i, minlength=ni)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k) + [(a, b) for a, b in extra]
    t = _trainer(conf, active, MB, [("window_hot_sub", sub), ("window_hot_max", 20 * sub), ("window_per_target", 100000)])
    ds = t.dataset_from_triples(u, i, r)
    W = ds.num_batches
    assert ds.kind == 8 and cnt.max() / W > 2 * sub, (cnt.max(), W)       # the top item takes several sub-steps per window
    assert W <= -(-cnt.max() // (20 * sub)) * 4
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    o = _substep_oracle(conf, active, u, i, r, W, sub, passes)
    for name in NAMES:
        assert np.isfinite(t.view(name)).all(), name
    _same_model(t, o, what=W)


def test_ten_random_wide_configurations_against_the_checker():
    """a slice of tests/fuzz_wide_window.py: widths 257 .. 1024, links, decays, sub-steps, caps, uniform and Zipf items"""
    import fuzz_wide_window
    from oracle import oracle
    oracle.build()
    rng = np.random.default_rng(18)
    assert all([fuzz_wide_window.one(rng, case) for case in range(10)])


# ------------------------------------------------------------------------------------------------- 6. scoring
def _check_scores(t, ds, d, labels):
    """predict_dataset == predict_batch of the same rows in file order; the evaluator against those predictions (tests/test_gpu_window_scoring.py)"""
    want = t.predict_batch(d)
    got = t.predict_dataset(ds)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    ss, cnt = t.eval_dataset(ds)
    assert cnt == len(want)
    diff = (got - np.asarray(labels, np.float32)).astype(np.float64)
    assert abs(ss - float(np.sum(diff * diff))) <= 1e-9 * ss
    return got


@pytest.mark.parametrize("k", [320, 1024])
@pytest.mark.parametrize("hot_sub", [0, 4])
def test_scoring_a_rating_sequence(k, hot_sub):
    nu, ni, n = 300, 60, 3000
    u, i, r = cases.planted_triples(n, nu, ni, seed=5, zipf=True)
    assert np.bincount(i[:700]).max() > 40
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    d = CSRData.from_triples(u, i, r)
    models = []
    for score_between in (True, False):   # train -> score -> train equals train -> train
        t = _trainer(conf, 0, MB + [("amd:window", 700)], [("window_hot_sub", hot_sub)])
        ds = t.dataset_from_triples(u, i, r)
        assert ds.kind == 8 and ds.num_batches == 5
        t.train_dataset(ds)
        if score_between:
            _check_scores(t, ds, d, r)
        t.train_dataset(ds)
        t.synchronize()
        models.append({nm: t.view(nm).copy() for nm in NAMES})
    for nm in NAMES:
        assert np.array_equal(models[0][nm].view(np.uint32), models[1][nm].view(np.uint32)), nm


@pytest.mark.parametrize("k", [320, 1024])
def test_scoring_a_pair_sequence_and_stand_alone_windows(k):
    nu, ni, n = 200, 50, 2000
    pu, pp, pq = cases.planted_pairs(n, nu, ni, seed=k)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k)
    t = _trainer(conf, 3, MB + [("amd:window", 600)])
    ds = t.dataset_from_pairs(pu, pp, pq)
    assert ds.kind == 8 and ds.num_batches == 4
    t.train_dataset(ds)
    ones = np.ones(n, np.float32)
    _check_scores(t, ds, sa.pairs_as_csr(pu, pp, pq), ones)
    win = t.dataset_window_from_pairs(pu, pp, pq)
    assert win.kind == 5
    _check_scores(t, win, sa.pairs_as_csr(pu, pp, pq), ones)
    # a stand-alone rating window, before and after the first half of the window step
    u, i, r = cases.planted_triples(900, 150, 40, seed=3)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=150, num_item=40, num_factor=k)
    d = CSRData.from_triples(u, i, r)
    t = _trainer(conf)
    t.train_dataset(t.dataset_from_triples(u, i, r))   # an exact pass first: the model is not the initial one
    win = t.dataset_window_from_triples(u, i, r)
    assert win.kind == 5
    before = _check_scores(t, win, d, r)
    t.train_dataset(win)
    after = _check_scores(t, win, d, r)
    assert not np.array_equal(before, after)


# ------------------------------------------------------------------------------------------------- 7. routes
def test_auto_chooses_the_window_step_on_a_deep_file_at_a_wide_width():
    from test_gpu_auto_step import _grouped_pairs
    nu, ni = 120, 400
    cols = _grouped_pairs(nu, ni, 500, 7)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=320)
    models = []
    for step in ("auto", "minibatch"):
        t = _trainer(conf, 3, [("amd:step", step)])
        ds = t.dataset_from_pairs(*cols)
        assert ds.kind == 8
        if step == "auto":
            assert t.counter(16) == 2 and t.counter(18) > 2 * t.counter(19)
        for _ in range(2):
            t.train_dataset(ds)
        models.append({n: t.view(n).copy() for n in ("W_user", "W_item", "i_bias")})
    for n in models[0]:
        assert np.array_equal(models[0][n].view(np.uint32), models[1][n].view(np.uint32)), n


def test_staged_triples_take_the_window_step_and_rows_with_globals_stay_exact():
    import test_gpu_staged_window as sw
    nu, ni, n = 500, 40, 11000
    u, i, r = cases.planted_triples(n, nu, ni, seed=3, zipf=True)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=320)
    make = lambda extra: sw._trainer(conf, extra=list(extra), knobs=[("stage_window", sw.S)])
    # counter 30 == number of chunks, counter 31 == 0, the model == dataset_from_triples(chunk) + train_dataset chunk by chunk
    sw._check(make, d, lambda t, a, b: t.dataset_from_triples(u[a:b], i[a:b], r[a:b]), 1500, names=NAMES)
    # one global feature per row: the user-unit route stops at 256 factors, the chunk keeps the exact flush without an error
    from test_gpu_wunit import _rows_with_globals
    ng = 12
    g = _rows_with_globals(9500, 300, 50, ng, 1, seed=2, fixed=True)
    gconf = cases.conf_with(cases.BASICMF_CONF, num_user=300, num_item=50, num_global=ng, num_factor=320, wd_global="0.001")
    t = sw._trainer(gconf, extra=MB, knobs=[("stage_window", sw.S)])
    e = sw._trainer(gconf, knobs=[("stage_window", sw.S)])
    sw._feed(t, g, 1000)
    sw._feed(e, g, 1000)
    sw._same(sw._views(t), sw._views(e))
    assert t.counter(30) == 0 and t.counter(31) > 0


def test_virtual_ranks_of_an_amd_gpus_handle_at_a_wide_width():
    nu, ni, n, k, world, windows, passes = 600, 100, 8000, 320, 2, 2, 2
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    u, i, r = cases.planted_triples(n, nu, ni, seed=9)
    t = _trainer(conf, 0, [("amd:gpus", world), ("amd:delta_half", 0), ("amd:window", n // windows), ("amd:step", "minibatch")])
    for _ in range(passes):
        t.update_batch(CSRData.from_triples(u, i, r))
        t.finish_round()
    assert t.counter(8) == passes * windows and t.counter(11) == passes * windows
    sim = simulate(conf, u, i, r, world, windows, passes, minibatch=True)
    for name in ("W_item", "i_bias"):
        assert np.array_equal(t.view(name).view(np.uint32), sim[0].t.view(name).view(np.uint32)), name
    wu, bu = t.view("W_user"), t.view("u_bias")
    for rk in range(world):
        own = (np.arange(nu) % world) == rk
        assert np.array_equal(wu[own].view(np.uint32), sim[rk].t.view("W_user")[own].view(np.uint32))
        assert np.array_equal(bu[own].view(np.uint32), sim[rk].t.view("u_bias")[own].view(np.uint32))


# ------------------------------------------------------------------------------------------------- 8. refusals that stay
def test_refusals_that_stay():
    u, i, r = cases.planted_triples(100, 50, 20, seed=1)
    t = sa.Trainer(0, 0)
    for k, v in cases.conf_with(cases.BASICMF_CONF, num_user=50, num_item=20, num_factor=1025):
        t.set_param(k, str(v))
    with pytest.raises(sa.SvdfError, match="num_factor > 1024"):
        t.init_model()
        t.init_trainer()
    pu, pp, pq = cases.planted_pairs(200, 50, 20, seed=1)
    pconf = cases.conf_with(cases.PAIR_CONF, num_user=50, num_item=20, num_factor=320)
    t = _trainer(pconf, 3, MB, [("window_pair_sub", 8)])
    with pytest.raises(sa.SvdfError, match="window_pair_sub > 0 needs num_factor <= 256"):
        t.dataset_from_pairs(pu, pp, pq)
    from test_gpu_wunit import _rows_with_globals
    g = _rows_with_globals(200, 50, 20, 4, 1, seed=2, fixed=True)
    gconf = cases.conf_with(cases.BASICMF_CONF, num_user=50, num_item=20, num_global=4, num_factor=320)
    with pytest.raises(sa.SvdfError, match="num_factor <= 256"):
        _trainer(gconf).dataset_window_from_csr(g)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=50, num_item=20, num_factor=320)
    with pytest.raises(sa.SvdfError, match="window data sets"):
        _trainer(conf + [("reg_method", "4")]).dataset_window_from_triples(u, i, r)


# ------------------------------------------------------------------------------------------------- 9. the accuracy contract
def test_the_window_step_keeps_the_accuracy_contract_at_a_wide_width():
    """Zipf items, 300 000 ratings in windows of 3 000 with the default lane of ordered sub-steps (window_hot_sub = 128; the top item has about 164
    slots per window), k = 320, three passes: held-out RMSE within 1e-4 of the exact pass -- the contract of every window step.  The checkers alone
    on the CPU (svdo_update_window_substeps(d, 128) per window against svdo_update_csr_batch) give exact 0.736855, window 0.736908, a difference of
    5.3e-5 (5.25e-5 at k = 64 on the same input); both engine paths equal their checkers bit for bit, so the figures printed here are those."""
    nu, ni, n, k = 20000, 2000, 300000, 320
    u, i, r = cases.planted_triples(n + 30000, nu, ni, seed=21, zipf=True)
    test = CSRData.from_triples(u[n:], i[n:], r[n:])
    tl = r[n:]
    u, i, r = u[:n], i[:n], r[:n]
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    out = []
    for extra in ([], MB + [("amd:window", 3000)]):
        t = _trainer(conf, 0, extra)
        ds = t.dataset_from_triples(u, i, r)
        for _ in range(3):
            t.train_dataset(ds)
        p = t.predict_batch(test)
        assert np.isfinite(p).all()
        out.append((float(np.sqrt(np.mean((p.astype(np.float64) - tl) ** 2))), ds.num_batches, ds.kind))
    print("held-out RMSE: exact %.6f window %.6f difference %.3g (%d windows)" % (out[0][0], out[1][0], out[1][0] - out[0][0], out[1][1]))
    assert out[1][2] == 8 and out[1][1] == 100
    assert abs(out[1][0] - out[0][0]) <= 1e-4, out

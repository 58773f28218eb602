"""Rank-pair rounds drawn from a candidate file (input_type = 2, svdf_dataset_from_rank_buffer_file) under `amd:step = minibatch` / `auto` on a
one-GPU handle: a file of plain unit-value rows is drawn in HBM by the device sampler AND cut into rank-pair windows there
-- a kind-8 sequence of kind-5 windows, the sequence svdf_dataset_from_pairs builds from the same pairs -- with libc's generator left where the
host sampler leaves it.

Expected pairs: the host sampler on a host-only handle (rank_sample_buffer_file; tests/test_rank_sampler.py pins it to the reference's generator).
Expected parameters: the pair-window checker of the one-GPU pair tests, tests/multi_rank_utils.py on one rank -- the pinned C port's update per row
on the window-start state, summed per item in file order -- never the library under test.  Window counts: svdf_dataset_from_pairs on a
format_type = 0 trainer given the same pairs and knobs (host columns, the host form of the window rule)."""
import numpy as np
import pytest

import cases
import multi_rank_utils
import svdfeature_amd as sa
from svdfeature_amd import data as D
from svdfeature_amd.data import TAG_DEFAULT, CSRData, PlusBlock

pytestmark = pytest.mark.gpu

NU, NI = 60, 50
SEED = 10
C_DEVICE_PASSES, C_AUTO, C_WINDOW_PASSES = 7, 16, 37
I_CHILD_KIND = 8
VIEWS = ("W_user", "W_item", "u_bias", "i_bias", "W_ufeedback", "ufeedback_bias")
E = (np.zeros(0, np.uint32), np.zeros(0, np.float32))


def _conf(k=8, **kw):
    """RANK_E2E_CONF without globals: num_ufeedback = 50, so the user rows sit behind a feedback space (user_off != 0)"""
    base = [(a, b) for a, b in cases.RANK_E2E_CONF if a not in ("num_global", "wd_global")] + [("num_global", "0")]
    return tuple(cases.conf_with(base, num_factor=k, **kw))


def _plain_blocks(seed, nblocks=600):
    """the blocks of cases.rank_blocks(nblocks, 60, 50, 0, seed, side_user=False, max_fb=0) -- 0 .. 8 candidate rows, labels 0 / 1 -- as PLAIN rows:
    one user entry, the row's first item entry, both values 1; an item named twice in a block moves to the next free id (a positive and a negative row
    of one item would merge into a one-entry pair, which the pair windows refuse)"""
    out = []
    for b in cases.rank_blocks(nblocks, NU, NI, 0, seed, side_user=False, max_fb=0):
        rows, used = [], set()
        for r in range(b.data.num_row):
            label, ng, nu, _, ix, _ = b.data.row(r)
            uid, i = int(ix[ng]), int(ix[ng + nu])
            while i in used:
                i = (i + 1) % NI
            used.add(i)
            rows.append((label, [], [(uid, 1.0)], [(i, 1.0)]))
        out.append(PlusBlock(E[0], E[1], CSRData.from_rows(rows) if rows else CSRData.empty(), TAG_DEFAULT))
    return out


def _burst_blocks(seed):
    """the base file with 100 consecutive blocks whose only positive row is item 7, next to 8 negatives: ~800 consecutive pairs that all name item 7"""
    blocks = _plain_blocks(seed)
    for j in range(100):
        neg = [(7 + 1 + (3 * j + m) % (NI - 1)) % NI for m in range(8)]
        rows = [(1.0, [], [(j % NU, 1.0)], [(7, 1.0)])] + [(0.0, [], [(j % NU, 1.0)], [(i, 1.0)]) for i in dict.fromkeys(neg)]
        blocks[200 + j] = PlusBlock(E[0], E[1], CSRData.from_rows(rows), TAG_DEFAULT)
    return blocks


def _write(tmp_path, blocks, name="cand.buffer"):
    src = str(tmp_path / name)
    D.write_ugroup_buffer(src, blocks)
    return src


def _trainer(conf, extra=(), knobs=(), device=-1):
    t = sa.Trainer(1, 3, device=device)
    t.seed(SEED)
    for k, v in tuple(conf) + tuple(extra):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


def _pairs_of(blocks):
    """(user, positive item, negative item) of one drawn pass: rows of label 1, user:1, two item entries in index order, the
    negative's value sign-flipped (apex_svd_data.cpp:828-860, 905-911)"""
    ba = sa.BlockArrays.from_blocks(blocks)
    n = ba.num_row
    if n == 0:
        z = np.zeros(0, np.uint32)
        return z, z, z
    base, rp = 3 * np.arange(n), np.asarray(ba.row_ptr)
    assert np.array_equal(rp[0:3 * n:3], base) and np.array_equal(rp[1::3], base) and np.array_equal(rp[2::3], base + 1) and rp[-1] == 3 * n
    idx, val = ba.feat_index.reshape(n, 3), ba.feat_value.reshape(n, 3)
    assert np.all(val[:, 0] == 1.0) and np.all(np.abs(val[:, 1:]) == 1.0) and np.all(val[:, 1] == -val[:, 2]) and np.all(ba.row_label == 1.0)
    first = val[:, 1] > 0
    return idx[:, 0].copy(), np.where(first, idx[:, 1], idx[:, 2]).astype(np.uint32), np.where(first, idx[:, 2], idx[:, 1]).astype(np.uint32)


def _host_passes(src, conf, rounds, tmp_path):
    """the passes the HOST sampler draws from src after the same seed, keys and model initialisation: per round (user, pos, neg), the generated blocks
    and the next four rand() values"""
    h = _trainer(conf, device=-2)
    out = []
    for r in range(rounds):
        dst = str(tmp_path / ("host_pass_%d.buffer" % r))
        n = h.rank_sample_buffer_file(src, dst)
        blocks = D.read_ugroup_buffer(dst)
        u, p, q = _pairs_of(blocks)
        assert len(u) == n
        out.append((u, p, q, blocks, tuple(sa.rand_peek(4))))
    h.close()
    return out


def _run(src, conf, rounds, extra=(), knobs=(), prefetch=False, score=False):
    """rounds of (draw, train) on the engine; what the tests compare"""
    t = _trainer(conf, extra, knobs)
    res = {"kinds": [], "child": [], "rows": [], "windows": [], "peek": [], "pred": []}
    for r in range(rounds):
        t.set_round(r)
        if prefetch:
            t.rank_prefetch_buffer_file(src)
        ds = t.dataset_from_rank_buffer_file(src)
        res["peek"].append(tuple(sa.rand_peek(4)))
        res["kinds"].append(ds.kind)
        res["child"].append(ds.info(I_CHILD_KIND))
        res["rows"].append(ds.info(0))
        res["windows"].append(ds.num_batches)
        if score:
            res["pred"].append(t.predict_dataset(ds))
        t.train_dataset(ds)
        t.finish_round()
        ds.close()
    t.synchronize()
    res["views"] = {n: (None if t.view(n) is None else t.view(n).copy()) for n in VIEWS}
    res["counters"] = {c: t.counter(c) for c in (C_DEVICE_PASSES, C_AUTO, C_WINDOW_PASSES)}
    t.close()
    return res


def _checker(conf, passes, windows, bf16=False):
    """tests/multi_rank_utils.py on one rank: per round set_round, every window's pairs through the port's update on the window-start item side (a
    pair = a block of one row without feedback: update(block) == update_inner(row), apex_svd_base.h:557-561), the sums added at the window's end"""
    multi_rank_utils.CONTRIB_BF16 = bf16
    try:
        a = multi_rank_utils.OracleShard(multi_rank_utils.make_oracle(list(conf), SEED, 1, 3), minibatch=True)
    finally:
        multi_rank_utils.CONTRIB_BF16 = False
    for r, ((u, p, q, _, _), W) in enumerate(zip(passes, windows)):
        a.t.set_round(r)
        d = sa.pairs_as_csr(u, p, q)
        n = len(u)
        for w in range(W):
            a.delta_begin()
            a.train([PlusBlock(E[0], E[1], d.slice_rows(j, j + 1), TAG_DEFAULT) for j in range(n * w // W, n * (w + 1) // W)])
            a.delta_set(a.delta_get().copy())
        a.t.finish_round()
    return a.t


def _same_views(got, want_trainer, what=""):
    for n in VIEWS:
        w = want_trainer.view(n)
        g = got[n]
        if w is None or w.size == 0:
            assert g is None or g.size == 0, (n, what)
            continue
        assert g is not None and np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w, np.float32).view(np.uint32)), (n, what)


def _same_runs(a, b, what=""):
    assert a["kinds"] == b["kinds"] and a["child"] == b["child"] and a["rows"] == b["rows"] and a["windows"] == b["windows"], (what, a["kinds"], b["kinds"], a["child"], b["child"])
    assert a["peek"] == b["peek"], what
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    for n in VIEWS:
        x, y = a["views"][n], b["views"][n]
        assert (x is None) == (y is None), (what, n)
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, n)


MB = (("amd:step", "minibatch"),)


# ------------------------------------------------------------------------------------------------- 1. the key is honoured
def test_minibatch_is_honoured_on_a_file_the_device_sampler_takes(tmp_path):
    """three rounds under amd:step = minibatch: every pass is a kind-8 sequence of kind-5 pair windows built on the device (counter 37), holds the
    host sampler's pairs, and leaves libc's generator where the host sampler leaves it"""
    src = _write(tmp_path, _plain_blocks(901))
    conf = _conf()
    host = _host_passes(src, conf, 3, tmp_path)
    assert all(len(p[0]) > 1000 for p in host)
    got = _run(src, conf, 3, extra=MB)
    assert got["kinds"] == [8, 8, 8] and got["child"] == [5, 5, 5], (got["kinds"], got["child"])
    assert got["counters"][C_WINDOW_PASSES] == 3 and got["counters"][C_DEVICE_PASSES] == 3
    assert got["rows"] == [len(p[0]) for p in host]
    assert got["peek"] == [p[4] for p in host]


# ------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("contrib", ["fp32", "bf16"])
@pytest.mark.parametrize("reg", [0, 1])
@pytest.mark.parametrize("nub", [1, 0])
@pytest.mark.parametrize("k", [8, 64, 100, 256, 320])
def test_parameters_equal_the_pair_window_checker_bit_for_bit(k, nub, reg, contrib, tmp_path):
    """two rounds, amd:window = 250 pairs (4 .. 6 windows of the ~1 200 pairs of a pass), sigmoid rank link: every parameter view as uint32 against
    the checker on the host sampler's pairs cut at n w / W; k = 320 is a wide row"""
    src = _write(tmp_path, _plain_blocks(902))
    conf = _conf(k, no_user_bias=nub, reg_method=reg)
    host = _host_passes(src, conf, 2, tmp_path)
    got = _run(src, conf, 2, extra=MB + (("amd:window", 250), ("amd:contrib", contrib)))
    assert got["kinds"] == [8, 8] and got["child"] == [5, 5] and got["counters"][C_WINDOW_PASSES] == 2
    want_w = [-(-len(p[0]) // 250) for p in host]
    assert got["windows"] == want_w and all(4 <= w <= 6 for w in want_w), (got["windows"], want_w)
    assert got["rows"] == [len(p[0]) for p in host]
    _same_views(got["views"], _checker(conf, host, want_w, contrib == "bf16"), (k, nub, reg, contrib))


# ------------------------------------------------------------------------------------------------- 3. window counts
def _pair_windows(conf, passes, extra=(), knobs=()):
    """num_batches of svdf_dataset_from_pairs on a format_type = 0 trainer, the same pairs and knobs: the host form of the window rule"""
    plain = [(a, b) for a, b in conf if a not in ("format_type", "num_ufeedback", "wd_ufeedback", "ufeedback_init_sigma", "input_type")]
    t = sa.Trainer(0, 3)
    t.seed(SEED)
    for a, b in tuple(plain) + MB + tuple(extra):
        t.set_param(a, str(b))
    t.init_model()
    t.init_trainer()
    for a, b in knobs:
        t.set_knob(a, b)
    out = []
    for u, p, q, _, _ in passes:
        ds = t.dataset_from_pairs(u, p, q)
        assert ds.kind == 8
        out.append(ds.num_batches)
        ds.close()
    t.close()
    return out


@pytest.mark.parametrize("case", ["default", "burst", "per_target_max", "amd_window"])
def test_window_counts_equal_those_of_dataset_from_pairs(case, tmp_path):
    """the device forms of the item counts, the per-pass rule and its raise on the windows as cut give the W of the host forms: on the base file, on a
    file where ~800 consecutive pairs name one item (the as-cut rule raises W above the per-pass count -- on the host side too), with
    window_per_target_max lowered, and with amd:window set"""
    src = _write(tmp_path, _burst_blocks(903) if case == "burst" else _plain_blocks(903))
    conf = _conf()
    extra = (("amd:window", 300),) if case == "amd_window" else ()
    knobs = (("window_per_target_max", 16),) if case == "per_target_max" else ()
    host = _host_passes(src, conf, 2, tmp_path)
    want = _pair_windows(conf, host, extra, knobs)
    got = _run(src, conf, 2, extra=MB + extra, knobs=knobs)
    print(case, "windows", got["windows"], "dataset_from_pairs", want)
    assert got["child"] == [5, 5] and got["counters"][C_WINDOW_PASSES] == 2
    assert got["windows"] == want
    if case == "burst":
        per_pass = _pair_windows(conf, host, extra, (("window_count_actual", 0),))
        print("per-pass rule alone", per_pass)
        assert all(a > b for a, b in zip(want, per_pass)), (want, per_pass)
    if case == "amd_window":
        assert want == [-(-len(p[0]) // 300) for p in host]


# ------------------------------------------------------------------------------------------------- 4. declines
def _decline_case(case, tmp_path):
    """(candidate file, conf, extra keys, knobs, prefetch)"""
    blocks, conf, extra, knobs, prefetch = _plain_blocks(904, 300), _conf(), MB, (), False
    if case == "non_unit_value":
        d = blocks[7].data
        v = d.feat_value.copy()
        v[-1] = 0.5
        blocks[7] = PlusBlock(E[0], E[1], CSRData(d.row_label, d.row_ptr, d.feat_index, v), TAG_DEFAULT)
    elif case == "feedback_ids":
        blocks[5] = PlusBlock(np.array([3, 9], np.uint32), np.full(2, 1.0 / np.sqrt(2.0), np.float32), blocks[5].data, TAG_DEFAULT)
    elif case == "global_entry":
        conf = tuple(cases.conf_with(list(conf), num_global=8, wd_global="0.001"))
        d = blocks[7].data
        rows = []
        for r in range(d.num_row):
            label, ng, nu, _, ix, va = d.row(r)
            rows.append((label, [(2, 0.5)] if r == 0 else [], [(int(ix[0]), 1.0)], [(int(ix[1]), 1.0)]))
        blocks[7] = PlusBlock(E[0], E[1], CSRData.from_rows(rows), TAG_DEFAULT)
    elif case == "window_pair_sub":
        knobs = (("window_pair_sub", 8),)
    elif case == "reg_method_4":   # lazy decay: amd:step = minibatch refuses it on this input with or without the route (the test below pins that);
        # the run that trains is `auto`'s, which keeps such a configuration exact
        conf, extra = tuple(cases.conf_with(list(conf), reg_method=4)), (("amd:step", "auto"),)
    elif case == "prefetch":
        prefetch = True
    assert blocks[7].data.num_row > 0 and blocks[5].data.num_row > 0
    return _write(tmp_path, blocks), conf, extra, knobs, prefetch


@pytest.mark.parametrize("case", ["non_unit_value", "feedback_ids", "global_entry", "window_pair_sub", "reg_method_4", "prefetch", "device_window_0"])
def test_what_the_route_declines_trains_as_before(case, tmp_path):
    """outside the route's conditions the call does what it did: kinds, counters, rand() positions and parameter bits equal those of a trainer kept off
    the route by knob device_window = 0; nothing raises and counter 37 stays 0"""
    src, conf, extra, knobs, prefetch = _decline_case(case, tmp_path)
    off = _run(src, conf, 2, extra=extra, knobs=knobs + (("device_window", 0),), prefetch=prefetch)
    got = _run(src, conf, 2, extra=extra, knobs=knobs + ((("device_window", 0),) if case == "device_window_0" else ()), prefetch=prefetch)
    assert got["counters"][C_WINDOW_PASSES] == 0 and 5 not in got["child"], (got["counters"], got["child"])
    assert all(n > 100 for n in got["rows"])
    _same_runs(got, off, case)


def test_lazy_decay_under_minibatch_keeps_its_refusal(tmp_path):
    """reg_method = 4 with amd:step = minibatch: the window step has no lazy decay and says so, as it did before the route existed"""
    src = _write(tmp_path, _plain_blocks(904, 300))
    t = _trainer(tuple(cases.conf_with(list(_conf()), reg_method=4)), MB)
    with pytest.raises(sa.SvdfError, match="window data sets: no side tables, relaxed ids, lazy decay or shared latent space"):
        t.dataset_from_rank_buffer_file(src)
    assert t.counter(C_WINDOW_PASSES) == 0
    t.close()


# ------------------------------------------------------------------------------------------------- 5. auto
def test_auto_takes_the_route_after_the_pass_that_decided(tmp_path):
    """amd:step = auto: the first pass goes through the level schedule and decides as before (counter 16 == 2: the window step), passes two and
    three are built on the device; the draws are those of a run without the key"""
    src = _write(tmp_path, _plain_blocks(905))
    conf = _conf()
    plain = _run(src, conf, 3)
    got = _run(src, conf, 3, extra=(("amd:step", "auto"),))
    assert got["counters"][C_AUTO] == 2, got["counters"]
    assert got["kinds"] == [8, 8, 8] and got["child"][1:] == [5, 5], (got["kinds"], got["child"])
    assert got["counters"][C_WINDOW_PASSES] == 2
    assert got["rows"] == plain["rows"] and got["peek"] == plain["peek"] and min(got["rows"]) > 1000
    for n in ("W_user", "W_item", "i_bias"):
        a, b = plain["views"][n], got["views"][n]
        assert np.isfinite(b).all() and np.abs(a - b).max() < 0.05, n   # (the bound of tests/test_gpu_auto_step.py for this input)


# ------------------------------------------------------------------------------------------------- 6. scoring
def test_predictions_come_in_file_order_and_equal_predict_block(tmp_path):
    """svdf_predict_dataset on such a sequence == svdf_predict_block on the drawn rows, bit for bit, on a trained model; svdf_eval_dataset agrees with
    those predictions; scoring between two passes changes nothing"""
    src = _write(tmp_path, _plain_blocks(906))
    conf = _conf(64)
    extra = MB + (("amd:window", 300),)
    host = _host_passes(src, conf, 2, tmp_path)
    t = _trainer(conf, extra)
    for r in range(2):
        t.set_round(r)
        ds = t.dataset_from_rank_buffer_file(src)
        assert ds.kind == 8 and ds.info(I_CHILD_KIND) == 5 and ds.num_batches > 1
        if r == 1:
            got = t.predict_dataset(ds)
            want = np.concatenate([t.predict_block(b) for b in host[1][3] if b.data.num_row > 0])
            assert got.shape == want.shape and len(got) == len(host[1][0])
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, "%d of %d predictions differ from predict_block, first at file row %d" % (bad.size, len(got), bad[0])
            ss, cnt = t.eval_dataset(ds)
            diff = (got - np.float32(1.0)).astype(np.float64)
            ref = float(np.sum(diff * diff))
            print("eval: ss %.17g from the predictions %.17g" % (ss, ref))
            assert cnt == len(got) and abs(ss - ref) <= 1e-9 * ss
        t.train_dataset(ds)
        t.finish_round()
        ds.close()
    t.synchronize()
    scored = {n: (None if t.view(n) is None else t.view(n).copy()) for n in VIEWS}
    t.close()
    plain = _run(src, conf, 2, extra=extra)
    for n in VIEWS:
        assert (scored[n] is None) == (plain["views"][n] is None)
        if scored[n] is not None:
            assert np.array_equal(scored[n].view(np.uint32), plain["views"][n].view(np.uint32)), n


# ------------------------------------------------------------------------------------------------- 7. edges
def _edge_blocks(case):
    if case == "zero_pairs":     # no negative row anywhere: every block is skipped by the sampler
        return [PlusBlock(E[0], E[1], CSRData.from_rows([(1.0, [], [(b, 1.0)], [(i, 1.0)]) for i in range(b % 5 + 1)]), TAG_DEFAULT) for b in range(20)]
    if case == "one_block":
        return [PlusBlock(E[0], E[1], CSRData.from_rows([(float(i % 2), [], [(3, 1.0)], [(i, 1.0)]) for i in range(7)]), TAG_DEFAULT)]
    blocks = _plain_blocks(907, 40)
    blocks[11] = PlusBlock(E[0], E[1], CSRData.from_rows([(1.0, [], [(9, 1.0)], [(i, 1.0)]) for i in range(6)]), TAG_DEFAULT)
    return blocks


@pytest.mark.parametrize("case", ["zero_pairs", "one_block", "all_positive_block"])
def test_edges(case, tmp_path):
    """a pass that draws no pair (one window without instances: training and scoring it are no-ops), a file of one block, a block without negatives"""
    src = _write(tmp_path, _edge_blocks(case))
    conf = _conf()
    host = _host_passes(src, conf, 2, tmp_path)
    got = _run(src, conf, 2, extra=MB, score=True)
    assert got["kinds"] == [8, 8] and got["child"] == [5, 5] and got["counters"][C_WINDOW_PASSES] == 2
    assert got["rows"] == [len(p[0]) for p in host] and got["peek"] == [p[4] for p in host]
    assert (got["rows"] == [0, 0]) == (case == "zero_pairs")
    assert [len(p) for p in got["pred"]] == got["rows"]
    _same_views(got["views"], _checker(conf, host, got["windows"]), case)
    assert got["windows"] == ([1, 1] if case == "zero_pairs" else _pair_windows(conf, host))


# ------------------------------------------------------------------------------------------------- 8. no key
def test_without_the_key_the_pass_stays_exact(tmp_path):
    src = _write(tmp_path, _plain_blocks(908))
    got = _run(src, _conf(), 2)
    assert got["kinds"] == [2, 2] and got["child"] == [-1, -1]
    assert got["counters"][C_WINDOW_PASSES] == 0 and got["counters"][C_DEVICE_PASSES] == 2

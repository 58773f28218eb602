"""`amd:step = minibatch` on the STAGED route of a one-GPU handle (svdf_update_csr / _csr_batch / _block; svdf_staged.cpp).
The semantics are defined by equivalence: a chunk -- the rows staged between two flush points -- trains as

    ds = svdf_dataset_from_X(t, chunk); svdf_train_dataset(t, ds); svdf_dataset_destroy(ds)

would on the same handle state, X picked from the chunk's rows (triples / pairs / csr / blocks).  Every test builds the resident side chunk by
chunk from the cuts the staging makes and compares every parameter view bit for bit; the inputs repeat items inside a window, so that the
window result differs from the exact (default step) result -- asserted, which is what tells this route from the exact flush.  Counter 30
counts the chunks the window step trained, 31 the chunks kept exact because rows or configuration are outside it."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_START

pytestmark = pytest.mark.gpu

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")
S = 4096   # knob stage_window of the tests: several chunks and a remainder at finish_round


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


def _views(t, names=VIEWS):
    t.synchronize()
    return {n: t.view(n).copy() for n in names if t.view(n).size}


def _same(a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)), n


def _differ(a, b):
    return any(not np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in a)


def _feed(t, d, batch):
    """batch > 0: svdf_update_csr_batch calls of `batch` rows; 0: one svdf_update_csr call per instance"""
    if batch:
        for s in range(0, d.num_row, batch):
            t.update_batch(d.slice_rows(s, s + batch))
    else:
        for r in range(d.num_row):
            t.update_csr(*d.row(r))
    t.finish_round()


def _cuts(n, batch, window):
    """the chunks the staging makes: a flush whenever `window` rows are staged after a call, the remainder at finish_round"""
    cuts, a, staged = [], 0, 0
    for s in range(0, n, batch or 1):
        staged += min(batch or 1, n - s)
        if staged >= window:
            cuts.append((a, a + staged))
            a, staged = a + staged, 0
    if staged:
        cuts.append((a, a + staged))
    return cuts


def _resident(t, d, cuts, build):
    for a, b in cuts:
        ds = build(t, a, b)
        assert ds.kind == 8
        t.train_dataset(ds)
        ds.close()
    return t


def _check(make, d, build, batch, window=S, names=VIEWS, min_chunks=2):
    """staged under the key == resident chunk by chunk, != the default step; counters 0 and 30"""
    cuts = _cuts(d.num_row, batch, window)
    assert len(cuts) >= min_chunks
    t = make([("amd:step", "minibatch")])
    _feed(t, d, batch)
    r = _resident(make([("amd:step", "minibatch")]), d, cuts, build)
    e = make([])
    _feed(e, d, batch)
    got, want, exact = _views(t, names), _views(r, names), _views(e, names)
    assert all(np.isfinite(v).all() for v in got.values())
    _same(got, want)
    assert _differ(got, exact), "the staged window step returned the exact (default step) bits"
    assert t.counter(30) == len(cuts) and t.counter(31) == 0
    assert t.counter(0) == r.counter(0) == d.num_row
    assert e.counter(30) == 0 and e.counter(31) == 0
    return t


def _from_csr(d):
    return lambda t, a, b: t.dataset_from_csr(d.slice_rows(a, b))


# ------------------------------------------------------------------------------------------------ plain ratings: wseq_from_triples
@pytest.mark.parametrize("zipf,batch,async_flush,window_key", [(False, 1000, 1, None), (False, 0, 0, None), (True, 1500, 0, None), (True, 0, 1, None),
                                                              (True, 2500, 1, 900)])
def test_plain_ratings_take_the_triples_sequence(zipf, batch, async_flush, window_key):
    """uniform items, and Zipf items whose head has more than window_hot_sub (128) ratings per window: the hot lane (k_window_apply) runs.
    window_key: `amd:window` instead of the knob -- chunk size and rows per window"""
    nu, ni, n = 500, 40, 11000
    u, i, r = cases.planted_triples(n, nu, ni, seed=3, zipf=zipf)
    if zipf:
        assert np.bincount(i[:S]).max() > 128
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32)
    knobs = [("async_flush", async_flush)] + ([] if window_key else [("stage_window", S)])
    make = lambda extra: _trainer(conf, extra=list(extra) + ([("amd:window", window_key)] if window_key else []), knobs=knobs)
    _check(make, d, lambda t, a, b: t.dataset_from_triples(u[a:b], i[a:b], r[a:b]), batch, window=window_key or S,
           names=("W_user", "u_bias", "W_item", "i_bias"))


def test_the_default_window_rule_applies_to_the_chunks_own_counts():
    """no window size given: one chunk at finish_round, cut into the windows the resident rule asks for on the chunk's item counts"""
    nu, ni, n = 500, 40, 9000
    u, i, r = cases.planted_triples(n, nu, ni, seed=5)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32)
    make = lambda extra: _trainer(conf, extra=extra)
    t = _check(make, d, lambda t, a, b: t.dataset_from_triples(u[a:b], i[a:b], r[a:b]), 3000, window=1 << 21, names=("W_user", "u_bias", "W_item", "i_bias"),
               min_chunks=1)
    w = make([("amd:step", "minibatch")]).dataset_from_triples(u, i, r).num_batches
    assert w > 1 and t.counter(2) == w   # one batch per window


# ------------------------------------------------------------------------------------------------ rank pairs: wseq_from_pairs
@pytest.mark.parametrize("batch,async_flush", [(700, 1), (0, 0)])
def test_generator_shaped_pairs_take_the_pair_sequence(batch, async_flush):
    nu, ni, per_user = 90, 60, 100
    rng = np.random.default_rng(7)
    u = np.repeat(np.arange(nu, dtype=np.uint32), per_user)   # the generator's order: user-grouped
    p = rng.integers(0, ni, len(u)).astype(np.uint32)
    q = ((p + 1 + rng.integers(0, ni - 1, len(u))) % ni).astype(np.uint32)
    d = sa.pairs_as_csr(u, p, q)
    conf = cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=32)
    make = lambda extra: _trainer(conf, active=3, extra=extra, knobs=[("stage_window", S), ("async_flush", async_flush)])
    _check(make, d, lambda t, a, b: t.dataset_from_pairs(u[a:b], p[a:b], q[a:b]), batch, names=("W_user", "W_item", "i_bias"))


# ------------------------------------------------------------------------------------------------ everything else: wseq_from_csr
@pytest.mark.parametrize("batch,async_flush", [(1000, 1), (0, 0)])
def test_rows_with_globals_take_the_csr_sequence(batch, async_flush):
    from test_gpu_wunit import _rows_with_globals
    nu, ni, ng = 300, 50, 12
    d = _rows_with_globals(9500, nu, ni, ng, 3, seed=2, fixed=True)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=ng, num_factor=32, wd_global="0.001")
    make = lambda extra: _trainer(conf, extra=extra, knobs=[("stage_window", S), ("async_flush", async_flush)])
    _check(make, d, _from_csr(d), batch)


NP, NS, NT, NA, NG = 200, 12, 40, 10, 5


def _shared_conf(k=32):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NT + NA, num_global=NG, num_factor=k, wd_global="0.002", learning_rate="0.01")


@pytest.mark.parametrize("sub,batch", [(0, 1000), (12, 1000), (12, 0)])
def test_shared_user_entries_and_ordered_sub_steps(sub, batch):
    """rows with shared user entries under amd:shared_user_from (12 shared ids: every one is hot); window_shared_sub = 12 applies them in
    ordered sub-steps (k_wunit_apply_shared)"""
    d = ws.shared_rows(np.random.default_rng(4), 9000, NP, NS, NT, num_global=NG, max_g=2, max_shared=2, uvals=True)
    knobs = [("stage_window", S), ("window_shared_sub", sub)]
    make = lambda extra: _trainer(_shared_conf(), extra=list(extra) + [("amd:shared_user_from", NP)], knobs=knobs)
    _check(make, d, _from_csr(d), batch)


@pytest.mark.parametrize("batch,async_flush,window_key", [(1000, 0, None), (0, 1, None), (350, 1, 100)])
def test_feature_user_and_feature_item_tables(tmp_path, batch, async_flush, window_key):
    rng = np.random.default_rng(6)
    tu = ws.read_table(ws.write_table(str(tmp_path / "fu.txt"), ws.random_table(rng, NP + NS, NP, NP + NS, 2)))
    ti = ws.read_table(ws.write_table(str(tmp_path / "fi.txt"), ws.random_table(rng, NT, NT, NT + NA, 2)))
    d = ws.table_rows(rng, 9000, NP, NS, NT, num_global=NG, max_g=2, max_shared=1, max_items=2, uvals=True, ivals=True)
    d = ws.drop_rows_reaching_twice(d, NP, tu, ti)
    conf = _shared_conf() + [("feature_user", str(tmp_path / "fu.txt")), ("feature_item", str(tmp_path / "fi.txt"))]
    knobs = [("async_flush", async_flush)] + ([] if window_key else [("stage_window", S)])
    make = lambda extra: _trainer(conf, extra=list(extra) + [("amd:shared_user_from", NP)] + ([("amd:window", window_key)] if window_key else []), knobs=knobs)
    _check(make, d, _from_csr(d), batch, window=window_key or S)


@pytest.mark.parametrize("batch,async_flush", [(1000, 1), (0, 0)])
def test_a_mixed_chunk_takes_from_csr(batch, async_flush):
    """plain (user, item) rows followed by rows with globals inside ONE chunk: neither triples nor pairs, the chunk goes through wseq_from_csr"""
    from test_gpu_wunit import _rows_with_globals
    nu, ni, ng = 300, 50, 12
    u, i, r = cases.planted_triples(3000, nu, ni, seed=8)
    d = CSRData.concat([CSRData.from_triples(u, i, r), _rows_with_globals(3000, nu, ni, ng, 3, seed=9, fixed=True)])
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=ng, num_factor=32, wd_global="0.001")
    make = lambda extra: _trainer(conf, extra=extra, knobs=[("stage_window", S), ("async_flush", async_flush)])
    _check(make, d, _from_csr(d), batch)


# ------------------------------------------------------------------------------------------------ user-group trainers: wseq_from_blocks
SVDPP = [("num_ufeedback", 60), ("wd_ufeedback", "0.004")]


def _block_cuts(blocks, window):
    """the automatic flush waits for the open user's END once `window` rows are staged"""
    cuts, a, staged = [], 0, 0
    for j, b in enumerate(blocks):
        staged += b.data.num_row
        if staged >= window and b.extend_tag in (TAG_DEFAULT, TAG_END):
            cuts.append((a, j + 1))
            a, staged = j + 1, 0
    if a < len(blocks):
        cuts.append((a, len(blocks)))
    return cuts


def test_user_group_blocks_with_users_straddling_the_window():
    nu, ni = 900, 60
    blocks = cases.user_blocks(850, nu, ni, 60, seed=12, max_rows=9, max_fb=6, split_every=2)
    window = 1000
    cuts = _block_cuts(blocks, window)
    rows = np.cumsum([b.data.num_row for b in blocks])
    # some automatic flush point falls inside a START .. END span: the chunk ends later than the row count alone would end it
    assert len(cuts) >= 3 and any(blocks[b - 1].extend_tag == TAG_END and rows[b - 2] - (rows[a - 1] if a else 0) >= window for a, b in cuts[:-1])
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32) + SVDPP
    make = lambda extra: _trainer(conf, fmt=1, extra=extra, knobs=[("stage_window", window)])
    names = ("W_user", "u_bias", "W_item", "i_bias", "W_ufeedback", "ufeedback_bias")

    def feed(t):
        for b in blocks:
            t.update_block(b)
        t.finish_round()
        return t
    t, e = feed(make([("amd:step", "minibatch")])), feed(make([]))
    r = _resident(make([("amd:step", "minibatch")]), None, cuts, lambda t_, a, b: t_.dataset_from_blocks(BlockArrays.from_blocks(blocks[a:b])))
    got = _views(t, names)
    _same(got, _views(r, names))
    assert _differ(got, _views(e, names))
    assert t.counter(30) == len(cuts) and t.counter(31) == 0 and t.counter(0) == r.counter(0) == int(rows[-1])


def test_a_forced_flush_inside_a_user_keeps_that_user_exact():
    """finish_round with a user still open: the closed units train as a window sequence, the open tail -- and its continuation, first unit of the
    next chunk -- go through the exact unit path in file order"""
    nu, ni = 400, 60
    blocks = cases.user_blocks(300, nu, ni, 60, seed=13, max_rows=9, max_fb=6, split_every=2)
    j = next(x for x in range(100, len(blocks)) if blocks[x].extend_tag == TAG_START)   # a START block; MIDDLE and END follow
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32) + SVDPP
    make = lambda: _trainer(conf, fmt=1, extra=[("amd:step", "minibatch")])
    names = ("W_user", "u_bias", "W_item", "i_bias", "W_ufeedback", "ufeedback_bias")
    t = make()
    for b in blocks[:j + 1]:
        t.update_block(b)
    t.finish_round()
    for b in blocks[j + 1:]:
        t.update_block(b)
    t.finish_round()
    assert t.counter(30) == 2
    r = make()
    for a, b in ((0, j), (j + 3, len(blocks))):
        if a:   # the straddling user alone: an open unit, then its continuation -- the exact unit path, not counted as "outside the window step"
            r.update_block(blocks[j]); r.finish_round()
            r.update_block(blocks[j + 1]); r.update_block(blocks[j + 2]); r.finish_round()
        ds = r.dataset_from_blocks(BlockArrays.from_blocks(blocks[a:b]))
        r.train_dataset(ds)
        ds.close()
    assert r.counter(30) == 0 and r.counter(31) == 0 and t.counter(31) == 0
    _same(_views(t, names), _views(r, names))


# ------------------------------------------------------------------------------------------------ chunks outside the window step
def test_a_chunk_with_a_refused_row_trains_exactly_and_does_not_raise(capfd):
    """two user entries without amd:shared_user_from: the builders refuse the row; the chunk keeps the exact flush (the default step's bits),
    counter 31 counts it and one stderr line names the rule"""
    from test_gpu_wunit import _rows_with_globals
    nu, ni, ng = 300, 50, 12
    good = _rows_with_globals(6000, nu, ni, ng, 3, seed=2, fixed=True)
    bad = CSRData.from_rows([(3.0, [(1, 0.5)], [(5, 1.0), (9, 0.5)], [(7, 1.0)])])
    d = CSRData.concat([good.slice_rows(0, 5000), bad, good.slice_rows(5000, 6000)])
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=ng, num_factor=32, wd_global="0.001")
    make = lambda extra: _trainer(conf, extra=extra, knobs=[("stage_window", S)])
    t, e = make([("amd:step", "minibatch")]), make([])
    _feed(t, d, 1000)   # chunks: rows 0 .. 4999 (window step), the rest with the refused row (exact)
    assert t.counter(30) == 1 and t.counter(31) == 1
    err = capfd.readouterr().err
    assert err.count("keeps the exact") == 1 and "exactly one user entry" in err
    r = make([("amd:step", "minibatch")])
    ds = r.dataset_from_csr(d.slice_rows(0, 5000))
    r.train_dataset(ds)
    ds.close()
    with pytest.raises(sa.SvdfError):
        r.dataset_from_csr(d.slice_rows(5000, d.num_row))
    r.set_param("amd:step", "levels")
    r.update_batch(d.slice_rows(5000, d.num_row))
    r.finish_round()
    _same(_views(t), _views(r))
    _feed(e, d, 1000)
    assert _differ(_views(t), _views(e))


def test_a_configuration_outside_the_window_step_is_the_default_step(capfd):
    """lazy decay (reg_method 4): every chunk exact, bit for bit the handle without the key"""
    nu, ni = 300, 40
    u, i, r = cases.planted_triples(9000, nu, ni, seed=3)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32, reg_method=4)
    t = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=[("stage_window", S)])
    e = _trainer(conf, knobs=[("stage_window", S)])
    _feed(t, d, 1000)
    _feed(e, d, 1000)
    _same(_views(t), _views(e))
    assert t.counter(30) == 0 and t.counter(31) == len(_cuts(d.num_row, 1000, S)) == 2 and t.counter(1) == e.counter(1)
    assert capfd.readouterr().err.count("keeps the exact") == 1


def test_predict_between_updates_sees_the_flushed_state():
    nu, ni = 300, 40
    u, i, r = cases.planted_triples(6000, nu, ni, seed=3)
    d = CSRData.from_triples(u, i, r)
    probe = d.slice_rows(0, 64)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32)
    for async_flush in (0, 1):
        t = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=[("stage_window", S), ("async_flush", async_flush)])
        rr = _trainer(conf, extra=[("amd:step", "minibatch")], knobs=[("stage_window", S)])
        for s in range(0, 5000, 500):
            t.update_batch(d.slice_rows(s, s + 500))
        got = t.predict_batch(probe)          # a flush point: chunks [0, 4500) (automatic) and [4500, 5000)
        t.update_batch(d.slice_rows(5000, 6000))
        t.finish_round()
        for a, b in ((0, 4500), (4500, 5000)):
            ds = rr.dataset_from_triples(u[a:b], i[a:b], r[a:b])
            rr.train_dataset(ds)
            ds.close()
        want = rr.predict_batch(probe)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert t.counter(30) == 3


@pytest.mark.parametrize("extra", [(), (("amd:step", "levels"),)])
def test_without_the_key_and_with_levels_the_staged_route_is_the_reference(extra):
    """no key / amd:step = levels: the exact flush as before -- the C port of the reference bit for bit, no window chunk, no stderr"""
    from oracle import oracle
    oracle.build()
    nu, ni = 300, 40
    u, i, r = cases.planted_triples(9000, nu, ni, seed=3)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32)
    t = _trainer(conf, extra=extra, knobs=[("stage_window", S)])
    _feed(t, d, 1000)
    o = oracle.OracleTrainer("port", 0, 0)
    o.seed(10)
    for k, v in conf:
        o.set_param(k, v)
    o.init_model()
    o.init_trainer()
    o.update_batch(d)
    for n in ("W_user", "u_bias", "W_item", "i_bias"):
        assert np.array_equal(t.view(n).view(np.uint32), o.view(n).view(np.uint32)), n
    assert t.counter(30) == 0 and t.counter(31) == 0 and t.counter(32) == 0 and t.counter(3) == 2


def test_the_default_step_names_amd_step_auto_once_for_a_deep_staged_chunk(capfd):
    """the guard of the default step on the staged route: 12 000 ratings of ONE item are 12 000 levels (54 ms at 4.5 us each) against
    microseconds if they streamed -- one stderr line per handle, counter 32; counters 26 .. 28 (resident data sets) stay untouched"""
    nu, n = 12000, 12000
    u = np.arange(n, dtype=np.uint32)
    i = np.zeros(n, np.uint32)
    r = np.full(n, 4.0, np.float32)
    d = CSRData.from_triples(u, i, r)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=4, num_factor=8)
    t = _trainer(conf)
    for _ in range(2):
        t.update_batch(d)
        t.finish_round()
    t.synchronize()
    assert t.counter(32) == 1 and t.counter(26) == 0 and t.counter(27) == 0
    err = capfd.readouterr().err
    assert err.count("default (exact) step on staged rows") == 1 and "amd:step = auto" in err


def test_ordered_sub_steps_without_the_in_place_sums_keep_the_exact_step(capfd):
    """window_shared_sub > 0 with knob wunit_inplace = 0 is a configuration the builder refuses once a shared row is hot: decided before the
    build -- the chunks train exactly, nothing raises (neither here nor from the background flush)"""
    d = ws.shared_rows(np.random.default_rng(4), 9000, NP, NS, NT, num_global=NG, max_g=2, max_shared=2, uvals=True)
    knobs = [("stage_window", S), ("window_shared_sub", 12), ("wunit_inplace", 0), ("async_flush", 1)]
    t = _trainer(_shared_conf(), extra=[("amd:step", "minibatch"), ("amd:shared_user_from", NP)], knobs=knobs)
    e = _trainer(_shared_conf(), extra=[("amd:shared_user_from", NP)], knobs=knobs)
    _feed(t, d, 1000)
    _feed(e, d, 1000)
    _same(_views(t), _views(e))
    assert t.counter(30) == 0 and t.counter(31) == len(_cuts(d.num_row, 1000, S))
    assert "wunit_inplace" in capfd.readouterr().err


def test_a_user_that_never_closes_does_not_hold_the_flush_back_for_ever():
    """the automatic flush waits for the open user's END -- up to 4 x stage_window staged rows; beyond that the chunk is flushed as on the default
    route: the closed users before it as a window sequence, the open user through the exact unit path"""
    nu, ni, window = 300, 60, 200
    blocks = cases.user_blocks(120, nu, ni, 60, seed=14, max_rows=9, max_fb=6)
    rng = np.random.default_rng(15)
    uid, fb = nu - 1, np.arange(5, dtype=np.uint32)
    piece = lambda tag: sa.data.PlusBlock(fb if tag != 3 else fb[:0], np.full(5 if tag != 3 else 0, 0.4, np.float32),
                                         CSRData.from_triples(np.full(50, uid, np.uint32), rng.integers(0, ni, 50).astype(np.uint32),
                                                              rng.integers(1, 6, 50).astype(np.float32)), tag)
    long_user = [piece(TAG_START)] + [piece(3) for _ in range(30)] + [piece(TAG_END)]   # 1 600 rows in one START .. END span
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=32) + SVDPP
    t = _trainer(conf, fmt=1, extra=[("amd:step", "minibatch")], knobs=[("stage_window", window)])
    e = _trainer(conf, fmt=1, knobs=[("stage_window", window)])
    for x in (t, e):
        for b in blocks[:20] + long_user + blocks[20:]:
            x.update_block(b)
        x.finish_round()
    n = sum(b.data.num_row for b in blocks) + 1600
    assert t.counter(0) == e.counter(0) == n
    assert t.counter(3) > 4 and t.counter(30) >= 2      # flushed while the long user was open, not only at its END
    got = _views(t, ("W_user", "W_item", "W_ufeedback"))
    assert all(np.isfinite(v).all() for v in got.values())


def test_the_block_pool_changes_no_bit_and_serves_the_later_chunks():
    """knob staged_pool: the per-chunk sequences take their device blocks from the handle's pool (1, default) or from hipMalloc / hipFree (0)"""
    from test_gpu_wunit import _rows_with_globals
    nu, ni, ng = 300, 50, 12
    d = _rows_with_globals(9000, nu, ni, ng, 3, seed=2, fixed=True)
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=ng, num_factor=32, wd_global="0.001")
    got = []
    for mode in (0, 1):
        t = _trainer(conf, extra=[("amd:step", "minibatch"), ("amd:window", 300)], knobs=[("staged_pool", mode)])
        _feed(t, d, 1500)   # 6 chunks of 5 windows
        got.append(_views(t))
        assert t.counter(30) == 6
    _same(*got)

"""Run-major staging slots of the runs pass (svdf_runs.cpp: runs_stage_build, svdf_k_runs.hip: k_runs_operands / k_runs_label_rm and the STAGED form of
k_basicmf_runs_soa): operand j of the run at position s of the level order has slot number s * (1 + R) + j, so the dst words, the
biases and the labels of the 8 runs (4 at k = 128) a wave carries are one block each, loaded with one instruction each and handed to the lane groups by
cross-lane moves; the slot's row stays at row j * nunit + s of the row buffer, so every row store turns a slot number into that row.  Only addresses change: the model must equal, bit for bit, the pass on rows in W (runs_stage = 0) and the level-by-level pass over single instances
(runs_exec = 0) after one pass and after three, and the oracle after one.  The shapes are the smallest at which the block addressing can go wrong: levels
of fewer runs than a row set, of exactly one, of one more or less, partial last sets, every block size (runs_len 2 / 4 / 7: 24 / 40 / 64 dwords at
k = 64, 12 / 20 / 32 at k = 128), every launch shape."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_user", "W_item", "u_bias", "i_bias")
VARIANTS = {
    "staged": [("runs_exec", 1), ("runs_stage", 1)],
    "rows in W": [("runs_exec", 1), ("runs_stage", 0)],
    "levels of single instances": [("runs_exec", 0)],
}
UNITS, STAGE_STATE, STAGE_BYTES = 5, 9, 10
# never symmetric: different row decays, nonzero different bias decays, another learning rate and base score
ASYMMETRIC = dict(wd_user=0.02, wd_item=0.003, wd_user_bias=0.01, wd_item_bias=0.004, learning_rate=0.01, base_score=1.7)


def _setup(t, nu, ni, k, conf):
    t.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, **conf):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    return t


def _run(u, i, r, nu, ni, knobs, k, conf):
    """three passes -> (model after pass 1, after pass 3, data set)"""
    t = _setup(sa.Trainer(0, 0), nu, ni, k, conf)
    for kk, v in [("pivot_exec", 0), ("runs_min_rows", 0)] + knobs:
        t.set_knob(kk, v)
    ds = t.dataset_from_triples(u, i, r)
    t.train_dataset(ds)
    t.synchronize()
    first = {n: t.view(n).copy() for n in NAMES}
    t.train_dataset(ds)
    t.train_dataset(ds)
    t.synchronize()
    return first, {n: t.view(n).copy() for n in NAMES}, ds


def _same(a, b, what):
    for name in NAMES:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), (what, name)


def _check(u, i, r, nu, ni, knobs=(), k=64, conf=None):
    """the three passes agree after one pass and after three, the first equals the oracle; -> the staged data set"""
    from oracle import oracle
    oracle.build()
    conf = conf or {}
    got = {name: _run(u, i, r, nu, ni, kn + (list(knobs) if kn[0][1] else []), k, conf) for name, kn in VARIANTS.items()}
    assert [g[2].kind for g in got.values()] == [10, 10, 0]
    ref = got["staged"]
    assert ref[2].info(STAGE_STATE) == 1 and got["rows in W"][2].info(STAGE_STATE) == 0
    for name in list(VARIANTS)[1:]:
        _same(ref[0], got[name][0], name + ", one pass")
        _same(ref[1], got[name][1], name + ", three passes")
    o = _setup(oracle.OracleTrainer("port", 0, 0), nu, ni, k, conf)
    o.update_batch(sa.CSRData.from_triples(u, i, r))
    _same(ref[0], {n: o.view(n) for n in NAMES}, "the oracle, one pass")
    return ref[2]


def _two_levels(lengths, rl, seed):
    """Every user rates once.  Round 1: each of the len(lengths) items gets rl ratings -- one full run each, level 0.  Round 2, behind it in the file:
    item t gets lengths[t] <= rl more -- one run each, level 1, fed by level 0's item rows through the slots.  -> u, i, r, nu, ni"""
    rng = np.random.default_rng(seed)
    ni = len(lengths)
    i = np.concatenate([rng.permutation(np.repeat(np.arange(ni), rl)), rng.permutation(np.repeat(np.arange(ni), lengths))]).astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    return u, i, r, len(i), ni


@pytest.mark.parametrize("k,nrun", [(64, 3), (64, 7), (64, 8), (64, 9), (64, 17), (128, 3), (128, 4), (128, 5), (128, 9)])
@pytest.mark.parametrize("order", [0, 1])
def test_levels_around_one_row_set(k, nrun, order):
    """levels of fewer runs than one row set (8 runs at k = 64, 4 at k = 128), of exactly one, of one more and one less, of two and one: runs of every
    length, so that the partial last set of the length order holds the shortest"""
    lengths = np.random.default_rng(nrun).integers(1, 5, nrun)
    u, i, r, nu, ni = _two_levels(lengths, 4, seed=k + nrun)
    ds = _check(u, i, r, nu, ni, knobs=[("runs_order", order)], k=k)
    assert ds.num_batches == 2 and ds.info(UNITS) == 2 * nrun


@pytest.mark.parametrize("k,lengths", [(64, [4] * 8 + [2, 1, 1]), (64, [4] * 16 + [3, 1]), (128, [4] * 4 + [2, 1]), (128, [4] * 8 + [3, 1, 1])])
def test_partial_last_set_of_shorter_runs(k, lengths):
    """the lanes of a partial set past the level's end take the words of the set's first run -- here a longer run than the live ones behind it: they
    must load and store nothing, and the wave walks only the live runs' steps"""
    u, i, r, nu, ni = _two_levels(np.array(lengths), 4, seed=len(lengths))
    ds = _check(u, i, r, nu, ni, k=k)
    assert ds.num_batches == 2 and ds.info(UNITS) == 2 * len(lengths)


@pytest.mark.parametrize("k", [64, 128])
def test_all_runs_of_length_one(k):
    """every item is rated by one user only: a user's second rating of the item cannot join a run that holds its first"""
    ni = 37
    rng = np.random.default_rng(3)
    count = rng.integers(1, 30, ni)
    i = rng.permutation(np.repeat(np.arange(ni), count)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    ds = _check(i.copy(), i, r, ni, ni, k=k)
    assert ds.num_batches == int(count.max()) and ds.info(UNITS) == len(i)


@pytest.mark.parametrize("k,rl", [(64, 2), (64, 4), (64, 7), (128, 2), (128, 4), (128, 7)])
def test_all_runs_of_full_length(k, rl):
    """every user rates once and every item a multiple of runs_len times: full runs only, every lane of a block of 8 * (1 + 7) = 64 dwords in use"""
    ni, m = 29, 5
    rng = np.random.default_rng(4)
    i = rng.permutation(np.repeat(np.arange(ni), rl * m)).astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    ds = _check(u, i, r, len(i), ni, knobs=[("runs_len", rl)], k=k)
    assert ds.num_batches == m and ds.info(UNITS) == ni * m


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("rl", [2, 4, 7])
def test_every_block_size(k, rl):
    """mixed lengths up to runs_len, levels of up to 60 runs, rows handed on many times"""
    u, i, r = cases.planted_triples(12000, 700, 60, seed=10 + rl, zipf=True)
    _check(u, i, r, 700, 60, knobs=[("runs_len", rl)], k=k)


@pytest.mark.parametrize("knobs", [
    [("runs_sets", 2)],
    [("runs_sets", 2), ("runs_block", 256), ("xcd_remap", 1), ("runs_len", 7)],
    [("runs_block", 128), ("xcd_remap", 0)],
    [("runs_block", 128), ("xcd_remap", 1)],
    [("runs_block", 256), ("xcd_remap", 0)],
    [("runs_block", 256), ("xcd_remap", 1)],          # the grid is padded past the level's end
    [("runs_block", 256), ("xcd_remap", 1), ("runs_order", 0)],
    [("xcd_remap", 0), ("runs_order", 0)],
])
def test_launch_shapes(knobs):
    rng = np.random.default_rng(5)
    n, nu, ni = 20000, 900, 203   # levels of up to 203 runs: 25 row sets and a partial one, several blocks at every block size
    u, i, r = rng.integers(0, nu, n).astype(np.uint32), rng.integers(0, ni, n).astype(np.uint32), rng.integers(1, 6, n).astype(np.float32)
    _check(u, i, r, nu, ni, knobs=knobs)


def test_one_rating():
    _check(np.array([3], np.uint32), np.array([5], np.uint32), np.array([4.0], np.float32), 10, 8)


def test_a_user_rating_the_same_item_twice_in_a_row():
    rng = np.random.default_rng(3)
    nu, ni, n = 50, 12, 6000
    u = rng.integers(0, nu, n).astype(np.uint32)
    i = rng.integers(0, ni, n).astype(np.uint32)
    u[1::7] = u[0::7][:len(u[1::7])]     # the same (user, item) twice in a row, and the same user on consecutive ratings
    i[1::7] = i[0::7][:len(i[1::7])]
    r = rng.integers(1, 6, n).astype(np.float32)
    _check(u, i, r, nu, ni, knobs=[("runs_len", 7)])


@pytest.mark.parametrize("k", [64, 128])
def test_asymmetric_parameters(k):
    u, i, r = cases.planted_triples(15000, 1200, 150, seed=6, zipf=True)
    r = (r + np.random.default_rng(6).uniform(-0.5, 0.5, len(r)) - 2.25).astype(np.float32)   # real-valued labels, some negative
    _check(u, i, r, 1200, 150, k=k, conf=ASYMMETRIC)


def test_rows_never_touched_keep_their_bytes():
    nu, ni, n = 300, 50, 8000
    u, i, r = cases.planted_triples(n, 200, 30, seed=5)   # users 200 .., items 30 .. have no rating
    t = _setup(sa.Trainer(0, 0), nu, ni, 64, {})
    for kk, v in [("pivot_exec", 0), ("runs_min_rows", 0)] + VARIANTS["staged"]:
        t.set_knob(kk, v)
    before = {name: t.view(name).copy() for name in NAMES}
    ds = t.dataset_from_triples(u, i, r)
    for _ in range(3):
        t.train_dataset(ds)
    t.synchronize()
    assert ds.kind == 10 and ds.info(STAGE_STATE) == 1
    for name, cut in (("W_user", 200), ("u_bias", 200), ("W_item", 30), ("i_bias", 30)):
        after = t.view(name)
        assert np.array_equal(after[cut:].view(np.uint32), before[name][cut:].view(np.uint32)), name
        assert not np.array_equal(after[:cut].view(np.uint32), before[name][:cut].view(np.uint32)), name


def test_staging_bytes_count_the_label_copy():
    """rows + biases + dst words of (1 + R) slots per run, R labels per run, one first-slot word per row of W_user / W_item"""
    lengths = np.array([4, 3, 2, 1, 4, 4, 1, 2, 3])
    u, i, r, nu, ni = _two_levels(lengths, 4, seed=9)
    t = _setup(sa.Trainer(0, 0), nu, ni, 64, {})
    for kk, v in [("pivot_exec", 0), ("runs_min_rows", 0)] + VARIANTS["staged"]:
        t.set_knob(kk, v)
    ds = t.dataset_from_triples(u, i, r)
    units, slots = ds.info(UNITS), 5 * ds.info(UNITS)
    assert units == 18 and ds.info(STAGE_STATE) == 1
    assert ds.info(STAGE_BYTES) == slots * (4 * 64 + 8) + 4 * 4 * units + 4 * (nu + ni)   # a row of k = 64: 64 floats

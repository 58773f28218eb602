"""Store policy of the staged runs pass (knob runs_store; svdf_k_runs.hip: runs_store_row / runs_store_bias in the STAGED form of k_basicmf_runs_soa;
DESIGN.md section 2c): 0 = every store plain, 1 = the 4-byte bias words nontemporal and the rows plain, 2 = rows and bias words sc1 write-through;
and its gather with two user rows in flight.  A cache policy and the order in which loads are waited for change no bit: under every policy the staged pass must equal the pass on rows in W
(runs_stage = 0) and the level-by-level pass over single instances (runs_exec = 0) after one pass and after three, and the oracle after one.  The
references of a shape are computed once and shared by the three policies.  Shapes: the smallest at which a row set, a partial set or a store branch can
go wrong -- levels of fewer runs than a row set (8 runs at k = 64, 4 at k = 128), of exactly one, of one more, of two and one; partial last sets of
shorter runs; runs of one rating; full runs at every runs_len; rows touched exactly once (filled by k_runs_stage_in, their only store goes home); a
user rating an item twice in a row; every block size and tile mapping; asymmetric decays."""
import functools

import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_user", "W_item", "u_bias", "i_bias")
STAGED, IN_W, LEVELS = [("runs_exec", 1), ("runs_stage", 1)], [("runs_exec", 1), ("runs_stage", 0)], [("runs_exec", 0)]
UNITS, STAGE_STATE = 5, 9
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


def _two_levels(lengths, rl, seed):
    """Every user rates once: every user row is touched exactly once.  Round 1: each of the len(lengths) items gets rl ratings -- one full run each,
    level 0.  Round 2, behind it in the file: item t gets lengths[t] <= rl more -- one run each, level 1, fed by level 0's item rows through the slots."""
    rng = np.random.default_rng(seed)
    ni = len(lengths)
    i = np.concatenate([rng.permutation(np.repeat(np.arange(ni), rl)), rng.permutation(np.repeat(np.arange(ni), lengths))]).astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    return u, i, r, len(i), ni


def _level_case(k, nrun):
    lengths = np.random.default_rng(nrun).integers(1, 5, nrun)
    return _two_levels(lengths, 4, seed=k + nrun) + ([], k, {}, dict(levels=2, units=2 * nrun))


def _partial_case(k, lengths):
    return _two_levels(np.array(lengths), 4, seed=len(lengths)) + ([], k, {}, dict(levels=2, units=2 * len(lengths)))


def _length_one_case():
    """every item is rated by one user only: a user's second rating of the item cannot join a run that holds its first"""
    ni = 37
    rng = np.random.default_rng(3)
    count = rng.integers(1, 30, ni)
    i = rng.permutation(np.repeat(np.arange(ni), count)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    return i.copy(), i, r, ni, ni, [], 64, {}, dict(levels=int(count.max()), units=len(i))


def _full_length_case(k, rl):
    """every user rates once and every item a multiple of runs_len times: full runs only"""
    ni, m = 29, 5
    rng = np.random.default_rng(4)
    i = rng.permutation(np.repeat(np.arange(ni), rl * m)).astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    r = rng.integers(1, 6, len(i)).astype(np.float32)
    return u, i, r, len(i), ni, [("runs_len", rl)], k, {}, dict(levels=m, units=ni * m)


def _touched_once_case(k):
    """every user AND every item is rated exactly once: one level of runs of one rating, every slot filled by k_runs_stage_in, every store goes home;
    41 runs: five row sets and a partial one at k = 64"""
    rng = np.random.default_rng(8)
    n = 41
    u, i = rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32)
    r = rng.integers(1, 6, n).astype(np.float32)
    return u, i, r, n, n, [], k, {}, dict(levels=1, units=n)


def _twice_in_a_row_case():
    rng = np.random.default_rng(3)
    nu, ni, n = 50, 12, 6000
    u = rng.integers(0, nu, n).astype(np.uint32)
    i = rng.integers(0, ni, n).astype(np.uint32)
    u[1::7] = u[0::7][:len(u[1::7])]     # the same (user, item) twice in a row, and the same user on consecutive ratings
    i[1::7] = i[0::7][:len(i[1::7])]
    r = rng.integers(1, 6, n).astype(np.float32)
    return u, i, r, nu, ni, [("runs_len", 7)], 64, {}, {}


def _launch_case(block, remap):
    rng = np.random.default_rng(5)
    n, nu, ni = 20000, 900, 203   # levels of up to 203 runs: 25 row sets and a partial one, several blocks at every block size
    u, i, r = rng.integers(0, nu, n).astype(np.uint32), rng.integers(0, ni, n).astype(np.uint32), rng.integers(1, 6, n).astype(np.float32)
    return u, i, r, nu, ni, [("runs_block", block), ("xcd_remap", remap)], 64, {}, {}


def _asymmetric_case(k):
    u, i, r = cases.planted_triples(15000, 1200, 150, seed=6, zipf=True)
    r = (r + np.random.default_rng(6).uniform(-0.5, 0.5, len(r)) - 2.25).astype(np.float32)   # real-valued labels, some negative
    return u, i, r, 1200, 150, [], k, ASYMMETRIC, {}


CASES = {}
for _k, _n in [(64, 3), (64, 7), (64, 8), (64, 9), (64, 17), (128, 3), (128, 4), (128, 5), (128, 9)]:
    CASES["level of %d runs, k %d" % (_n, _k)] = functools.partial(_level_case, _k, _n)
CASES["partial last set of shorter runs, k 64"] = functools.partial(_partial_case, 64, [4] * 8 + [2, 1, 1])
CASES["partial last set of shorter runs, k 128"] = functools.partial(_partial_case, 128, [4] * 4 + [2, 1])
CASES["all runs of length 1"] = _length_one_case
for _rl in (2, 4, 7):
    CASES["full runs, runs_len %d" % _rl] = functools.partial(_full_length_case, 64, _rl)
CASES["full runs, runs_len 7, k 128"] = functools.partial(_full_length_case, 128, 7)
CASES["every row touched once, k 64"] = functools.partial(_touched_once_case, 64)
CASES["every row touched once, k 128"] = functools.partial(_touched_once_case, 128)
CASES["the same item twice in a row"] = _twice_in_a_row_case
for _b in (128, 256):
    for _x in (0, 1):
        CASES["runs_block %d, xcd_remap %d" % (_b, _x)] = functools.partial(_launch_case, _b, _x)
CASES["asymmetric decays, k 64"] = functools.partial(_asymmetric_case, 64)
CASES["asymmetric decays, k 128"] = functools.partial(_asymmetric_case, 128)


@functools.lru_cache(maxsize=None)
def _references(name):
    """the shape's data and, computed once for its three policies: the pass on rows in W and the level-by-level pass after one pass and after three,
    the oracle after one.  Nothing here is written again."""
    from oracle import oracle
    oracle.build()
    u, i, r, nu, ni, knobs, k, conf, want = CASES[name]()
    in_w = _run(u, i, r, nu, ni, IN_W + knobs, k, conf)
    levels = _run(u, i, r, nu, ni, LEVELS, k, conf)
    assert (in_w[2].kind, levels[2].kind) == (10, 0) and in_w[2].info(STAGE_STATE) == 0
    o = _setup(oracle.OracleTrainer("port", 0, 0), nu, ni, k, conf)
    o.update_batch(sa.CSRData.from_triples(u, i, r))
    refs = {"rows in W": in_w[:2], "levels of single instances": levels[:2], "the oracle": ({n: o.view(n).copy() for n in NAMES}, None)}
    _same(in_w[0], refs["the oracle"][0], "the references disagree: rows in W, the oracle")
    for pair in refs.values():
        for model in pair:
            for a in (model or {}).values():
                a.setflags(write=False)
    return (u, i, r, nu, ni, knobs, k, conf, want), refs


@pytest.mark.parametrize("store", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_every_policy_gives_the_same_bits(name, store):
    (u, i, r, nu, ni, knobs, k, conf, want), refs = _references(name)
    one, three, ds = _run(u, i, r, nu, ni, STAGED + knobs + [("runs_store", store)], k, conf)
    assert ds.kind == 10 and ds.info(STAGE_STATE) == 1
    if "levels" in want:
        assert ds.num_batches == want["levels"] and ds.info(UNITS) == want["units"]
    for what, (ref_one, ref_three) in refs.items():
        _same(one, ref_one, "runs_store %d against %s, one pass" % (store, what))
        if ref_three is not None:
            _same(three, ref_three, "runs_store %d against %s, three passes" % (store, what))


def test_the_policy_can_change_between_passes():
    """the knob is read at every pass: slots written under one policy are read after a pass under another, and the last pass's home stores too"""
    name = "runs_block 256, xcd_remap 1"
    (u, i, r, nu, ni, knobs, k, conf, _), refs = _references(name)
    t = _setup(sa.Trainer(0, 0), nu, ni, k, conf)
    for kk, v in [("pivot_exec", 0), ("runs_min_rows", 0)] + STAGED + knobs:
        t.set_knob(kk, v)
    ds = t.dataset_from_triples(u, i, r)
    for store in (2, 0, 1):
        t.set_knob("runs_store", store)
        t.train_dataset(ds)
    t.synchronize()
    _same({n: t.view(n).copy() for n in NAMES}, refs["rows in W"][1], "runs_store 2, 0, 1 over three passes")

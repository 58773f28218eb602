"""The runs kernel's gather and step loop (svdf_k_runs.hip): a lane group reads the item row and up to R user rows, slots beyond the
run's length and lane groups past the level's end read nothing and store nothing, the wave walks as many steps as its longest run.  The shapes below are
the smallest at which a change to that can go wrong: every run length with absent slots in every trailing position, levels that fill a wave partly /
exactly / by one run more (the second row set partly and wholly past the end), the first and the last row of W, rows nobody rates (they must keep their
initial bits: a redirected or range-checked load that goes wrong shows there), repeated users inside what would otherwise be one run.  Every case: 2 passes,
all four parameter arrays bit for bit against the level-by-level pass over single instances (runs_exec = 0) and against the oracle port trainer."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa

pytestmark = pytest.mark.gpu
NAMES = ("W_user", "W_item", "u_bias", "i_bias")
PASSES = 2


def _trainer(nu, ni, knobs, k):
    t = sa.Trainer(0, 0)
    t.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    t.set_knob("pivot_exec", 0)
    t.set_knob("runs_min_rows", 0)
    for kk, v in knobs:
        t.set_knob(kk, v)
    return t


def _run(u, i, r, nu, ni, knobs, k):
    t = _trainer(nu, ni, knobs, k)
    init = {n: t.view(n).copy() for n in NAMES}
    ds = t.dataset_from_triples(u, i, r)
    for _ in range(PASSES):
        t.train_dataset(ds)
    t.synchronize()
    return {n: t.view(n).copy() for n in NAMES}, init, ds, t


def _oracle(u, i, r, nu, ni, k):
    from oracle import oracle
    oracle.build()
    o = oracle.OracleTrainer("port", 0, 0)
    o.seed(10)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k):
        o.set_param(kk, v)
    o.init_model()
    o.init_trainer()
    data = sa.CSRData.from_triples(u, i, r)
    for _ in range(PASSES):
        o.update_batch(data)
    return {n: o.view(n).copy() for n in NAMES}


_REF = {}


def _reference(key, u, i, r, nu, ni, k):
    """(level-by-level pass, oracle) of one data set: computed once, shared by the cases that differ in knobs only, never written to"""
    if key not in _REF:
        plain, _, ds, _ = _run(u, i, r, nu, ni, [("runs_exec", 0)], k)
        assert ds.kind == 0
        orc = _oracle(u, i, r, nu, ni, k)
        for a in list(plain.values()) + list(orc.values()):
            a.setflags(write=False)
        _REF[key] = (plain, orc)
    return _REF[key]


def _check(key, u, i, r, nu, ni, knobs, k):
    plain, orc = _reference(key, u, i, r, nu, ni, k)
    got, init, ds, t = _run(u, i, r, nu, ni, [("runs_exec", 1)] + knobs, k)
    assert ds.kind == 10 and t.counter(23) == PASSES
    for name in NAMES:
        assert np.array_equal(got[name].view(np.uint32), plain[name].view(np.uint32)), (name, "runs_exec = 0")
        assert np.array_equal(got[name].view(np.uint32), orc[name].view(np.uint32)), (name, "oracle")
    return got, init, ds


def _form_runs(u, i, rf):
    """the rule of k_runs_form restated: lengths of the runs, item by item"""
    n = len(u)
    prev = np.full(n, -1, np.int64)
    last = {}
    for p in range(n):
        prev[p] = last.get(int(u[p]), -1)
        last[int(u[p])] = p
    lengths = []
    for it in np.unique(i):
        h, ln = -1, 0
        for p in np.flatnonzero(i == it):
            if 0 < ln < rf and (prev[p] < 0 or prev[p] < h):
                ln += 1
            else:
                if ln:
                    lengths.append(ln)
                h, ln = int(p), 1
        lengths.append(ln)
    return lengths


def _labels(n, seed):
    return np.random.default_rng(seed).integers(1, 6, n).astype(np.float32)


def _one_rating_per_user(counts, seed):
    """item t is rated counts[t] times, every rating by a user of its own, file order shuffled"""
    i = np.repeat(np.arange(len(counts)), counts)
    rng = np.random.default_rng(seed)
    i = i[rng.permutation(len(i))].astype(np.uint32)
    u = rng.permutation(len(i)).astype(np.uint32)
    return u, i, _labels(len(i), seed + 1)


# ---------------------------------------------------------------------------------------------- every run length
@pytest.mark.parametrize("rl,k", [(2, 64), (4, 64), (7, 64), (4, 128)])
def test_every_run_length(rl, k):
    """one rating per user, so any rating may join a run; item t has t + 1 ratings, t = 0 .. 2R: runs of every length 1 .. R, absent slots in every
    trailing position"""
    counts = np.arange(1, 2 * rl + 2)
    u, i, r = _one_rating_per_user(counts, seed=rl)
    hist = np.bincount(_form_runs(u, i, rl), minlength=rl + 1)
    want = np.zeros(rl + 1, np.int64)     # from the construction: c = a * R + b ratings are a full runs and, if b > 0, one of length b
    for c in counts:
        want[rl] += c // rl
        if c % rl:
            want[c % rl] += 1
    assert np.array_equal(hist, want) and (hist[1:] > 0).all()
    _, _, ds = _check(("len", rl, k), u, i, r, len(u), len(counts), [("runs_len", rl)], k)
    assert ds.num_units == hist.sum()


# ---------------------------------------------------------------------------------------------- partial and dead waves
def _level_data(k, rl=4):
    """levels of 9, 8, 7 and 1 runs at k = 64 (8 runs per wave and row set), of 5, 4, 3 and 1 at k = 128 (4 runs): with users of one rating each only an
    item's own runs follow one another, so level l holds one run of every item that has more than l runs"""
    runs_per_item = [4] + [3] * 6 + [2, 1] if k == 64 else [4, 3, 3, 2, 1]
    counts = np.array([(nr - 1) * rl + 1 + t % rl for t, nr in enumerate(runs_per_item)])   # full runs and a last one of 1 .. R ratings
    return runs_per_item, counts


@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("sets", [1, 2])
@pytest.mark.parametrize("k", [64, 128])
def test_partial_and_dead_waves(k, sets, block):
    runs_per_item, counts = _level_data(k)
    u, i, r = _one_rating_per_user(counts, seed=k)
    _, _, ds = _check(("lev", k), u, i, r, len(u), len(counts), [("runs_len", 4), ("runs_sets", sets), ("runs_block", block)], k)
    sizes = [sum(1 for nr in runs_per_item if nr > l) for l in range(max(runs_per_item))]
    assert sizes == ([9, 8, 7, 1] if k == 64 else [5, 4, 3, 1])
    assert ds.num_units == sum(runs_per_item) and ds.num_batches == len(sizes) and ds.max_batch == sizes[0]


# ---------------------------------------------------------------------------------------------- buffer edges
def _edge_data(rl):
    """nu = 6 R + 8 users, ni = 6 items.  The last item (the last row of W: items follow users) has a full run and a partial one, the full one with user
    nu - 1, the partial one with user 0; item 1 has a full and a partial run too, item 3 a single rating.  Users 1, nu - 2 and the multiples of 5, items
    0, 2 and ni - 2 are never rated."""
    nu, ni = 6 * rl + 8, 6
    free = iter([x for x in range(2, nu - 2) if x % 5 != 0])      # multiples of 5, 1 and nu - 2 stay unrated

    def take(c):
        return [next(free) for _ in range(c)]
    top_full = [nu - 1] + take(rl - 1)
    top_part = [0] + take(rl - 2)                                 # R - 1 ratings
    one_full = take(rl)
    one_part = take(max(1, rl - 2))
    single = take(1)
    u = top_full + top_part + one_full + one_part + single
    i = [ni - 1] * (len(top_full) + len(top_part)) + [1] * (len(one_full) + len(one_part)) + [3]
    assert len(set(u)) == len(u) and max(u) == nu - 1 and min(u) == 0
    # interleave the items in the file without changing any item's own order
    order = np.argsort(np.concatenate([np.arange(len(top_full) + len(top_part)) * 2, np.arange(len(one_full) + len(one_part)) * 2 + 1, [5]]), kind="stable")
    u, i = np.array(u, np.uint32)[order], np.array(i, np.uint32)[order]
    return u, i, _labels(len(u), 40 + rl), nu, ni


@pytest.mark.parametrize("rl,k", [(2, 64), (4, 64), (7, 64), (4, 128)])
def test_first_and_last_rows_and_rows_nobody_rates(rl, k):
    u, i, r, nu, ni = _edge_data(rl)
    lengths = sorted(_form_runs(u, i, rl))
    assert lengths.count(rl) == 2 and lengths[0] == 1 and len(lengths) == 5 and all(x < rl for x in lengths[:3])
    got, init, ds = _check(("edge", rl, k), u, i, r, nu, ni, [("runs_len", rl)], k)
    assert ds.num_units == 5
    idle_u = np.setdiff1d(np.arange(nu), u)
    idle_i = np.setdiff1d(np.arange(ni), i)
    assert {1, nu - 2} <= set(idle_u.tolist()) and set(idle_i.tolist()) == {0, 2, ni - 2}
    # a redirected load that became a store, or a range check off by one row, would show here
    assert np.array_equal(got["W_user"][idle_u].view(np.uint32), init["W_user"][idle_u].view(np.uint32))
    assert np.array_equal(got["u_bias"][idle_u].view(np.uint32), init["u_bias"][idle_u].view(np.uint32))
    assert np.array_equal(got["W_item"][idle_i].view(np.uint32), init["W_item"][idle_i].view(np.uint32))
    assert np.array_equal(got["i_bias"][idle_i].view(np.uint32), init["i_bias"][idle_i].view(np.uint32))
    # ... and the rated rows did move
    assert not np.array_equal(got["W_user"][[0, nu - 1]], init["W_user"][[0, nu - 1]])
    assert not np.array_equal(got["W_item"][ni - 1], init["W_item"][ni - 1])


# ---------------------------------------------------------------------------------------------- repeats
def _repeat_data():
    """item 0: users 10 11 11 12 13 ... (the same (user, item) twice in a row, file positions 1 and 2: the second one heads a new run); user 21 rates item 1
    at position 7 and item 2 at position 8 (the same user on consecutive ratings), and item 2's run was headed at position 5, before user 21's previous
    rating: the run is cut there.  Without the repeats each item's ratings would be one run of up to 7."""
    u = [10, 11, 11, 12, 13, 26, 20, 21, 21, 22, 23, 24, 25, 14, 15]
    i = [0, 0, 0, 0, 0, 2, 1, 1, 2, 2, 1, 2, 1, 0, 0]
    return np.array(u, np.uint32), np.array(i, np.uint32), _labels(len(u), 77), 30, 4


@pytest.mark.parametrize("rl,k", [(7, 64), (4, 64), (2, 64), (7, 128)])
def test_repeats_inside_what_would_be_one_run(rl, k):
    u, i, r, nu, ni = _repeat_data()
    lengths = _form_runs(u, i, 7)
    assert lengths == [2, 5, 4, 1, 3]   # items 0 and 2 are cut at the repeated user, item 1 is one run
    _, _, ds = _check(("rep", k), u, i, r, nu, ni, [("runs_len", rl)], k)
    assert ds.num_units == len(_form_runs(u, i, rl))

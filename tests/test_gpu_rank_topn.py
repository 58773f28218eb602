"""Top-N item lists on the live model (svdf_rank_topn, svdf_k_ranktopn.hip) on the GPU.  The checker is the numpy statement of
the rule in tests/test_rank_topn.py -- ids and the scores' bits must be equal -- and, for the agreement of the routes, svdf_rank_eval_positions
and the pinned port's ranker with top_k set."""
import ctypes as C

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from test_gpu_rank_eval import copy_model, new_trainer
from test_rank_topn import rule_topn

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = [1, 5, 16, 64, 100, 128, 200, 256, 320, 1024]
TOPS = [1, 10, 64, 100, 256]
NU, NI, NS = 300, 517, 203        # the item tile and the section tile are both ragged; four section tiles


def ptr_of(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)


def make_bans(S, nu, ni, seed, almost_all=30, keep=5, pool=None):
    """make_sections' recipe (tests/test_gpu_rank_eval.py) without positives: 0 - 40 banned items per section with duplicate entries; section
    `almost_all` bans all but `keep` items; user 7 in three sections; `pool`: the ids the bans of the sections 50 .. 59 are drawn from"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    users[[0, S // 4, S // 2]] = 7
    ban = []
    for s in range(S):
        perm = rng.permutation(ni)
        b = perm[keep:] if s == almost_all else perm[:int(rng.integers(0, 41))]
        if pool is not None and 50 <= s < 60:
            b = rng.permutation(pool)[:int(rng.integers(1, len(pool)))]
        if len(b) > 1:
            b = np.concatenate([b, b[:int(rng.integers(1, 4))]])   # duplicate ban entries count once
            b = b[rng.permutation(len(b))]
        ban.append(b.astype(np.uint32))
    return users, ptr_of(ban), np.concatenate(ban)


def model_of(t):
    return t.view("W_user").copy(), t.view("W_item").copy(), t.view("i_bias").copy()


def assert_same(got, want):
    """(items, scores, count, nan): ids, the scores' bits, counts and flags"""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[3], want[3])


_trained = {}


def trained(k):
    """the trained model of width k, its sections and its lists, computed once and shared (nothing below changes them)"""
    if k not in _trained:
        if k in (16, 128):
            t = new_trainer(NU, NI, k, conf=cases.PAIR_CONF, active=3)
            t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(4000, NU, NI, seed=k)))
        else:
            t = new_trainer(NU, NI, k)
            t.train_dataset(t.dataset_from_triples(*cases.planted_triples(4000, NU, NI, seed=k)))
        lists = make_bans(NS, NU, NI, seed=k)
        top_n = TOPS[KS.index(k) % len(TOPS)]
        before = t.counter(39)
        got = t.rank_topn(lists[0], top_n, lists[1], lists[2])
        _trained[k] = dict(t=t, lists=lists, top_n=top_n, got=got, counted=t.counter(39) - before)
    return _trained[k]


@pytest.mark.parametrize("k", KS)
def test_lists_equal_the_rule_on_random_trained_models(k):
    """every lane-group width and the wide rows; the model has been trained by one pass -- triples for most widths, rank pairs for k = 16 and
    128 -- so its rows are not the initial draw"""
    c = trained(k)
    users, ban_ptr, ban_item = c["lists"]
    U, W, bias = model_of(c["t"])
    want = rule_topn(U, W, bias, users, c["top_n"], ban_ptr, ban_item)
    assert want[2][30] == min(5, c["top_n"]) and(want[2] == np.minimum(c["top_n"], NI - np.array([len(np.unique(ban_item[a:b])) for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]))).all()
    assert_same(c["got"], want)
    assert c["counted"] == NS and not c["got"][3].any()
    if c["top_n"] > 5:
        assert (c["got"][0][30, 5:] == -1).all() and (c["got"][1][30, 5:] == 0).all()


@pytest.mark.parametrize("k", [64, 128])
def test_positions_of_the_listed_items_are_their_ranks(k):
    """svdf_rank_eval_positions on the same model: a section's list fed as its positives, with the same bans, comes back as 0, 1, 2, .. index
    for index, ties included (both routes break ties by id)"""
    c = trained(k)
    users, ban_ptr, ban_item = c["lists"]
    items, _, count, _ = c["got"]
    pos = [items[s, :count[s]].astype(np.uint32) for s in range(NS)]
    position, tied, ranked, nan = c["t"].rank_positions(users, ptr_of(pos), np.concatenate(pos), ban_ptr, ban_item)
    np.testing.assert_array_equal(position, np.concatenate([np.arange(n) for n in count]))
    assert not nan.any()


@pytest.mark.parametrize("k", [64, 128])
def test_lists_equal_the_port_rankers_top_k(k, tmp_path):
    """the pinned port's ranker with top_k = N on the saved model, fed as test_gpu_rank_eval.port_positions feeds it: the same list on every
    section whose N + 1 best scores are strictly decreasing (found by asking for N + 1); a section with fewer than N candidates is left out,
    the reference asserts there"""
    c = trained(k)
    t, N = c["t"], c["top_n"]
    users, ban_ptr, ban_item = c["lists"]
    items, _, count, _ = c["got"]
    more = t.rank_topn(users, N + 1, ban_ptr, ban_item)
    np.testing.assert_array_equal(more[0][:, :N], items)
    path = str(tmp_path / "m.model")
    t.save_model(path)
    r = oracle.OracleRanker("port", 0, 0)
    r.set_param("top_k", str(N))
    r.load_model(path)
    r.init_ranker(NI)
    r.process_rows(sa.CSRData.from_rows([(0.0, [], [], [(i, 1.0)]) for i in range(NI)]))
    compared = 0
    for s in range(NS):
        if count[s] < N:
            continue
        rows = [(2.0, [], [(int(users[s]), 1.0)], [])]
        b = ban_item[ban_ptr[s]:ban_ptr[s + 1]]
        if len(b):
            _, first = np.unique(b, return_index=True)
            rows.append((-1.0, [], [(int(x), 1.0) for x in np.asarray(b)[np.sort(first)]], []))
        rows.append((4.0, [], [], []))
        got = np.asarray(r.process_rows(sa.CSRData.from_rows(rows)))
        assert len(got) == N
        sc = more[1][s, :more[2][s]]
        if (np.diff(sc) < 0).all():
            compared += 1
            np.testing.assert_array_equal(got, items[s], err_msg=str(s))
    assert compared > 0.9 * NS


@pytest.mark.parametrize("k, ni", [pytest.param(7, 500, id="7"), pytest.param(64, 500, id="64"), pytest.param(128, 500, id="128"), pytest.param(200, 500, id="200"),
                                   pytest.param(320, 500, id="320"), pytest.param(64, 1200, id="64-1200items")])
def test_rounding_is_pinned(k, ni):
    """the clustered item rows of test_gpu_rank_eval.test_rounding_is_pinned (one base row +- 800 ulp per element): the scores of a section lie
    a few ulp apart -- condition asserted below: at least 20 % of the adjacent pairs within 4 ulp -- so the list depends on the summation
    order; it equals the rule in the pinned order and differs from the rule under a plain sequential sum.  With 1 200 items the sweep splits
    them over two workgroups in y and the merge has two lists."""
    nu, S, N = 40, 70, 50
    rng = np.random.default_rng(k)
    t = new_trainer(nu, ni, k)
    base = rng.standard_normal(k).astype(F32)
    bits = np.tile(base.view(np.int32), (ni, 1)) + rng.integers(-800, 801, (ni, k)).astype(np.int32)
    W = bits.view(F32)
    U = rng.standard_normal((nu, k)).astype(F32)
    bias = np.zeros(ni, F32)
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", bias)
    users, ban_ptr, ban_item = make_bans(S, nu, ni, seed=k + 1, almost_all=-1)
    close = total = 0
    for s in range(0, S, 7):
        sc = np.sort(U[users[s]].astype(np.float64) @ W.astype(np.float64).T)
        ulp = np.spacing(np.abs(sc[1:]).astype(F32)).astype(np.float64)
        close += int((np.diff(sc) < 4 * ulp).sum())
        total += len(sc) - 1
    assert close >= 0.2 * total, (close, total)
    got = t.rank_topn(users, N, ban_ptr, ban_item)
    assert_same(got, rule_topn(U, W, bias, users, N, ban_ptr, ban_item))
    other = rule_topn(U, W, bias, users, N, ban_ptr, ban_item, order="sequential")
    assert (got[0] != other[0]).any(axis=1).sum() >= 1          # the test sees the order


def pressure_model(case, nu, ni, k, rng):
    """small-integer models: every score is exact in fp32 in any summation order"""
    U = np.zeros((nu, k), F32)
    W = np.zeros((ni, k), F32)
    bias = np.zeros(ni, F32)
    ids = np.arange(ni, dtype=F32)
    if case in ("increasing", "decreasing"):
        U[:, 0] = 1.0 + np.arange(nu) % 3                      # score = (1 .. 3) * (+-id) + (u % 5): strictly monotone in the id
        U[:, 1] = 1.0
        W[:, 0] = ids if case == "increasing" else -ids
        W[:, 1] = 2.0
        bias[:] = 3.0
    elif case == "equal":
        U[:] = rng.integers(-2, 3, (nu, k))
        W[:] = rng.integers(-2, 3, k)[None, :]                  # one row for every item
        bias[:] = 1.0
    else:                                                       # "ties": test_gpu_rank_eval.test_ties_follow_the_documented_rule's model
        W[:] = rng.integers(-1, 2, (ni, k))
        U[:] = rng.integers(-1, 2, (nu, k))
        bias[:] = rng.integers(-1, 2, ni)
        W[:20] = 0.0
        W[5:10] = -0.0
        bias[:20] = np.where(np.arange(20) % 2 == 0, F32(0.0), F32(-0.0))
        W[20:30] = W[20]
        bias[20:30] = bias[20]                                  # ten copies of one item
        U[3] = 0.0                                              # a user every item ties for, up to the bias
    return U, W, bias


@pytest.mark.parametrize("case", ["increasing", "decreasing", "equal", "ties"])
def test_the_selection_under_pressure(case):
    """ni = 1200 (two workgroups in y), 70 sections (a full tile and a ragged one).  Scores strictly INCREASING with the id: every candidate
    beats the threshold, the most appends and cuts; strictly decreasing: none after the first top_n; all equal: the list is the top_n smallest
    unbanned ids; ties: zero rows with biases +-0 and ten copies of one item, bans drawn among the copies."""
    nu, ni, k, S = 30, 1200, 8, 70
    rng = np.random.default_rng(len(case))
    U, W, bias = pressure_model(case, nu, ni, k, rng)
    t = new_trainer(nu, ni, k)
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", bias)
    users, ban_ptr, ban_item = make_bans(S, nu, ni, seed=11, pool=np.arange(30) if case == "ties" else None)
    if case == "ties":
        users[40:44] = 3
    for N in (1, 100, 256):
        want = rule_topn(U, W, bias, users, N, ban_ptr, ban_item)
        assert_same(t.rank_topn(users, N, ban_ptr, ban_item), want)
        if case == "equal":
            s = 5
            left = np.setdiff1d(np.arange(ni), ban_item[ban_ptr[s]:ban_ptr[s + 1]])
            assert want[0][s].tolist() == left[:N].tolist()
        if case == "increasing":
            assert (np.diff(want[0][0, :want[2][0]]) < 0).all()


def test_nan_scores_flag_the_sections_that_rank_them():
    nu, ni, k, N = 20, 300, 12, 10
    t = new_trainer(nu, ni, k)
    t.train_dataset(t.dataset_from_triples(*cases.planted_triples(2000, nu, ni, seed=1)))
    clean = t.rank_topn(np.arange(4, dtype=np.uint32), N, [0, 0, 1, 3, 4], [123, 123, 123, 4])
    W = t.view("W_item")
    W[123] = np.nan
    t.set_view("W_item", W)
    users = np.arange(4, dtype=np.uint32)
    ban_ptr, ban_item = np.array([0, 0, 1, 3, 4], np.int64), np.array([123, 123, 123, 4], np.uint32)   # 0 ranks it, 1 bans it, 2 bans it twice, 3 bans another
    items, scores, count, nan = got = t.rank_topn(users, N, ban_ptr, ban_item)
    assert nan.tolist() == [1, 0, 0, 1] and count.tolist() == [0, N, N, 0]
    for s in (0, 3):
        assert (items[s] == -1).all() and (scores[s] == 0).all()
    for s in (1, 2):                                  # the sections that ban the row are what they were before it turned NaN
        np.testing.assert_array_equal(items[s], clean[0][s])
        np.testing.assert_array_equal(scores[s].view(np.uint32), clean[1][s].view(np.uint32))
    U, W, bias = model_of(t)
    assert_same(got, rule_topn(U, W, bias, users, N, ban_ptr, ban_item))


def test_end_to_end():
    nu, ni, k, S, N = 120, 700, 32, 150, 20
    u, i, r = cases.planted_triples(6000, nu, ni, seed=5)
    users, ban_ptr, ban_item = make_bans(S, nu, ni, seed=9)
    t = new_trainer(nu, ni, k)
    t.train_dataset(t.dataset_from_triples(u, i, r))
    got = t.rank_topn(users, N, ban_ptr, ban_item)      # straight after the unsynchronised pass: it must see the trained model
    t.synchronize()
    ref = new_trainer(nu, ni, k, seed=77)
    copy_model(t, ref)                                  # the trained model, read back after a synchronise, in another handle
    assert_same(got, ref.rank_topn(users, N, ban_ptr, ban_item))
    assert_same(got, rule_topn(*model_of(t), users, N, ban_ptr, ban_item))
    # ban_ptr = None is the same as empty ban lists
    none = t.rank_topn(users, N)
    assert_same(none, t.rank_topn(users, N, np.zeros(S + 1, np.int64), np.zeros(0, np.uint32)))
    assert (none[2] == N).all() and not np.array_equal(none[0], got[0])
    # in pieces of a few sections each: the workspace budget lowered to five lists
    before = t.counter(39)
    t.set_knob("rank_topn_budget", 5 * 512)
    assert_same(t.rank_topn(users, N, ban_ptr, ban_item), got)
    t.set_knob("rank_topn_budget", 1 << 25)
    assert t.counter(39) - before == S
    # no sections: nothing to do
    empty = t.rank_topn(np.zeros(0, np.uint32), N)
    assert empty[0].shape == (0, N) and t.counter(39) - before == S
    # score_out = NULL through the C entry point
    items, count, nan = np.zeros(S * N, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    rc = t.lib.svdf_rank_topn(t.h, S, users, ban_ptr.ctypes.data_as(C.c_void_p), ban_item.ctypes.data_as(C.c_void_p), N, items, None, count, nan)
    assert rc == 0
    np.testing.assert_array_equal(items.reshape(S, N), got[0])
    np.testing.assert_array_equal(count, got[2])
    # a window sequence of the same rows: the window step is not bit-equal to the exact pass, so the models are made identical through set_view
    w = new_trainer(nu, ni, k, extra=[("amd:step", "minibatch")])
    dw = w.dataset_from_triples(u, i, r)
    assert dw.kind == 8
    w.train_dataset(dw)
    gw = w.rank_topn(users, N, ban_ptr, ban_item)
    copy_model(w, ref)
    assert_same(gw, ref.rank_topn(users, N, ban_ptr, ban_item))
    assert not np.array_equal(gw[0], got[0])           # (and it IS another model)


def test_lists_are_refused_before_any_launch():
    t = new_trainer(20, 30, 8)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_topn([1, 2], 5, [0, 1, 2], [3, 30])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_topn([1, 2], 5, [0, 1, 2], [3, 4000000000])
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_topn([1, 20], 5)
    with pytest.raises(sa.SvdfError, match="ban_ptr must not decrease"):
        t.rank_topn([1, 2], 5, [0, 2, 1], [3, 4])
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_topn([1, 2], 257)
    assert t.counter(39) == 0
    items, scores, count, nan = t.rank_topn([1, 2], 40, [0, 3, 5], [7, 7, 8, 5, 5])
    assert count.tolist() == [28, 29] and t.counter(39) == 2 and items.shape == (2, 40)
    assert (items[0, :28] >= 0).all() and (items[0, 28:] == -1).all() and not set(items[0].tolist()) & {7, 8}

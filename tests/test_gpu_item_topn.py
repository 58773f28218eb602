"""Similar-item lists on the live model (svdf_item_topn, svdf_k_itemrows.hip) on the GPU.  The checker is the numpy statement
of the rule in tests/item_topn_rule.py -- ids and the scores' bits must be equal -- and, without numpy, svdf_rank_topn on a copy trainer
whose user rows are the query items' rows."""
import numpy as np
import pytest

import cases
from item_topn_rule import DECOYS, METRICS, edge_rows, pinned_case, random_rows, rule_similar, unit_rows
from rank_rounding import dot_fp32
from test_gpu_rank_eval import new_trainer
from test_gpu_rank_topn import KS, NI, NS, NU, TOPS, assert_same, make_bans, ptr_of

pytestmark = pytest.mark.gpu
F32 = np.float32
SELF_BAN = 3          # the section whose ban list holds its own query


def make_queries(S, ni, seed):
    """S query items, item 11 in three sections, with make_bans' ban lists (section 30 bans all but five items); section SELF_BAN also
    lists its own query among its bans, twice"""
    rng = np.random.default_rng(seed + 1)
    items = rng.integers(0, ni, S).astype(np.uint32)
    items[[0, S // 4, S // 2]] = 11
    _, ban_ptr, ban_item = make_bans(S, NU, ni, seed=seed)
    ban = [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    ban[SELF_BAN] = np.concatenate([ban[SELF_BAN], [items[SELF_BAN]] * 2]).astype(np.uint32)
    return items, ptr_of(ban), np.concatenate(ban)


def count_formula(items, ban_ptr, ban_item, top_n, ni):
    return np.array([min(top_n, ni - len(np.unique(np.concatenate([ban_item[a:b], [q]])))) for q, a, b in zip(items, ban_ptr[:-1], ban_ptr[1:])])


_trained = {}


def trained(k):
    """the trained model of width k (test_gpu_rank_topn's recipes: one pass of triples, rank pairs for k = 16 and 128), its sections and
    the lists of both metrics, computed once and shared (nothing below changes them)"""
    if k not in _trained:
        if k in (16, 128):
            t = new_trainer(NU, NI, k, conf=cases.PAIR_CONF, active=3)
            t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(4000, NU, NI, seed=k)))
        else:
            t = new_trainer(NU, NI, k)
            t.train_dataset(t.dataset_from_triples(*cases.planted_triples(4000, NU, NI, seed=k)))
        lists = make_queries(NS, NI, seed=k)
        top_n = TOPS[KS.index(k) % len(TOPS)]
        got, moved = {}, {}
        for metric in METRICS:
            before = t.counter(49), t.counter(39)
            got[metric] = t.similar_items(lists[0], top_n, metric, lists[1], lists[2])
            moved[metric] = t.counter(49) - before[0], t.counter(39) - before[1]
        _trained[k] = dict(t=t, lists=lists, top_n=top_n, got=got, moved=moved, W=t.view("W_item").copy())
    return _trained[k]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", KS)
def test_lists_equal_the_rule_on_random_trained_models(k, metric):
    """every lane-group width, both wide slot counts and ragged tails; 203 sections (four section tiles, the last ragged), an item queried
    three times, a section that bans all but five items, one that bans its own query; top_n cycles with k"""
    c = trained(k)
    items, ban_ptr, ban_item = c["lists"]
    want = rule_similar(c["W"], items, c["top_n"], metric, ban_ptr, ban_item)
    formula = count_formula(items, ban_ptr, ban_item, c["top_n"], NI)
    assert (want[2] == formula).all() and want[2][30] <= min(5, c["top_n"])
    got = c["got"][metric]
    assert_same(got, want)
    assert c["moved"][metric] == (NS, 0) and not got[3].any()
    for s in range(NS):
        assert items[s] not in got[0][s]


@pytest.mark.parametrize("metric", METRICS)
def test_all_items(metric):
    """items = None: every item once, in id order; top_n 256"""
    c = trained(64)
    got = c["t"].similar_items(None, 256, metric)
    assert got[0].shape == (NI, 256) and (got[2] == 256).all()
    assert_same(got, rule_similar(c["W"], np.arange(NI), 256, metric))
    assert_same(got, c["t"].similar_items(np.arange(NI, dtype=np.uint32), 256, {"dot": 0, "cosine": 1}[metric]))


@pytest.mark.parametrize("k", [5, 64, 320])
def test_dot_lists_equal_rank_topn_on_a_copy_trainer(k):
    """without numpy: a trainer whose W_user[s] is W_item[item[s]] and whose i_bias is zero; its rank_topn under the same bans plus the
    query gives the ids and score bits of similar_items(metric="dot")"""
    c = trained(k)
    items, ban_ptr, ban_item = c["lists"]
    ref = new_trainer(NS, NI, k, seed=77)
    ref.set_view("W_item", c["W"])
    ref.set_view("W_user", c["W"][items])
    ref.set_view("i_bias", np.zeros(NI, F32))
    ban = [np.concatenate([ban_item[a:b], [q]]).astype(np.uint32) for q, a, b in zip(items, ban_ptr[:-1], ban_ptr[1:])]
    assert_same(c["got"]["dot"], ref.rank_topn(np.arange(NS, dtype=np.uint32), c["top_n"], ptr_of(ban), np.concatenate(ban)))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [7, 64, 300])
def test_scores_are_symmetric(k, metric):
    """257 items, all of them queries, top_n 256: each list is complete, and the score bits of (q, i) and (i, q) are equal"""
    ni = 257
    t = new_trainer(40, ni, k)
    t.set_view("W_item", random_rows(ni, k, seed=100 + k))
    items, scores, count, nan = t.similar_items(None, 256, metric)
    assert (count == 256).all() and not nan.any()
    M = np.zeros((ni, ni), np.uint32)
    M[np.arange(ni)[:, None], items] = scores.view(np.uint32)
    np.testing.assert_array_equal(M, M.T)
    assert (M != 0).sum() > ni * 250


@pytest.mark.parametrize("k", [3, 64, 130, 320])
def test_unit_rows_on_the_device(k):
    """the exclusion hides a query's own cosine score, so item 9's row is planted under id 400 too: its score against the original is
    <R[9], R[9]> of the rule, bit for bit"""
    t = new_trainer(40, NI, k)
    W = random_rows(NI, k, seed=200 + k)
    W[400] = W[9]
    t.set_view("W_item", W)
    items, scores, count, nan = t.similar_items([9, 400], 1)
    R = unit_rows(W[9:10])
    want = F32(0.0) + (F32(0.0) + dot_fp32(R[0], R)[0])
    assert abs(float(want) - 1.0) <= 2 * float(np.spacing(F32(1.0)))       # a sanity check on the input, not the assertion
    assert items.tolist() == [[400], [9]] and not nan.any()
    assert scores.view(np.uint32).tolist() == [[want.view(np.uint32)]] * 2


@pytest.mark.parametrize("k", [7, 64, 130, 320])
def test_rounding_is_pinned(k):
    """the inputs tests/test_item_topn.py shows to tell the decoys apart (a reciprocal multiply, a sequential sum of squares, a float64
    norm): the GPU's lists equal the pinned rule and none of the three"""
    W = pinned_case(k)
    t = new_trainer(40, len(W), k)
    t.set_view("W_item", W)
    items = np.arange(0, len(W), 7)
    got = t.similar_items(items, 50)
    assert_same(got, rule_similar(W, items, 50))
    for d in DECOYS:
        other = rule_similar(W, items, 50, decoy=d)
        assert (other[0] != got[0]).any() or (other[1].view(np.uint32) != got[1].view(np.uint32)).any(), d


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [10, 300])
def test_edge_rows(k, metric):
    """an item table that holds the edge rows of the CPU test behind 40 random rows (40 zero, 41 -0, 42 underflowing squares, 43 denormal
    squares, 44 overflow, 45 a NaN, 46 an inf): every item is a query; the sections 0 .. 19 and 40 .. 44 ban both 45 and 46, the sections
    20 .. 24 only 45, the others nothing"""
    W = np.concatenate([random_rows(40, k, seed=300 + k), edge_rows(k)])
    ni = len(W)
    t = new_trainer(40, ni, k)
    t.set_view("W_item", W)
    ban = [np.array([45, 46] if s < 20 or 40 <= s < 45 else [45] if s < 25 else [], np.uint32) for s in range(ni)]
    ban_ptr, ban_item = ptr_of(ban), np.concatenate(ban)
    got = t.similar_items(None, 20, metric, ban_ptr, ban_item)
    want = rule_similar(W, np.arange(ni), 20, metric, ban_ptr, ban_item)
    assert_same(got, want)                               # every listed score bit for bit, the flags exactly where the rule sets them
    clean = np.r_[0:20, 40:45]
    assert not got[3][clean].any() and (got[2][clean] == 20).all()      # a banned NaN item does not flag
    assert got[3][25:40].all() and got[3][45] == 1                       # ranking the NaN row does, and so does being it
    if metric == "cosine":
        assert got[3][20:25].all()                                       # inf / inf: row 46's unit row holds a NaN
        assert not got[1][40:43].any() and got[0][40].tolist() == list(range(20))   # zero-norm queries score +0 against everything


@pytest.mark.parametrize("metric", METRICS)
def test_pieces_give_the_same_lists_and_build_the_unit_rows_once(metric):
    """rank_topn_budget lowered to five lists: pieces of five sections and one item range; the output is identical, and the launches are one
    gather, one sweep and one merge per piece plus -- cosine only -- ONE launch for the unit rows of the whole call"""
    c = trained(64)
    t, N = c["t"], c["top_n"]
    items, ban_ptr, ban_item = c["lists"]
    cap = t.rank_geometry("topn", NS, N)["cap"]
    t.synchronize()
    launches = []
    for budget in (1 << 25, 5 * cap):
        t.set_knob("rank_topn_budget", budget)
        before = t.counter(1)
        got = t.similar_items(items, N, metric, ban_ptr, ban_item)
        launches.append(t.counter(1) - before)
        assert_same(got, c["got"][metric])
    t.set_knob("rank_topn_budget", 1 << 25)
    once = 1 if metric == "cosine" else 0
    assert launches == [once + 3, once + 3 * ((NS + 4) // 5)]


def test_a_moved_model_is_seen():
    """call, train one more pass, call again: the second answer is the rule on the new model -- nothing of the first call's unit rows is left"""
    k = 32
    t = new_trainer(NU, NI, k)
    data = t.dataset_from_triples(*cases.planted_triples(4000, NU, NI, seed=5))
    t.train_dataset(data)
    items = np.arange(0, NI, 5, dtype=np.uint32)
    first = t.similar_items(items, 10)
    assert_same(first, rule_similar(t.view("W_item"), items, 10))
    t.train_dataset(data)
    second = t.similar_items(items, 10)          # straight after the unsynchronised pass
    assert_same(second, rule_similar(t.view("W_item"), items, 10))
    assert (first[1].view(np.uint32) != second[1].view(np.uint32)).any()


def test_rank_topn_is_unchanged_by_an_item_call():
    c = trained(64)
    t = c["t"]
    users, ban_ptr, ban_item = make_bans(NS, NU, NI, seed=64)
    c39, c49 = t.counter(39), t.counter(49)
    launched = t.counter(1)
    before = t.rank_topn(users, 10, ban_ptr, ban_item)
    per_call = t.counter(1) - launched
    assert t.counter(39) - c39 == NS and t.counter(49) == c49
    t.similar_items(users % NI, 10, "cosine", ban_ptr, ban_item)
    assert t.counter(39) - c39 == NS and t.counter(49) - c49 == NS
    launched = t.counter(1)
    assert_same(t.rank_topn(users, 10, ban_ptr, ban_item), before)
    assert t.counter(39) - c39 == 2 * NS and t.counter(1) - launched == per_call == 2

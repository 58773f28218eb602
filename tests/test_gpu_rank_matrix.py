"""The opt-in selecting sweep on the matrix cores (knob rank_topn_scores = 1, svdf_k_ranktopn_mfma.hip) on the GPU: exact
against int64 numpy on integer models, within the published bound of a float64 reference on float models, and the routes the knob reaches."""
import numpy as np
import pytest

import svdfeature_amd as sa
from test_gpu_rank_eval import new_trainer
from test_gpu_rank_topn import assert_same, make_bans, ptr_of
from test_rank_feedback import NFB, fb_conf
from test_rank_lines import lines_conf

pytestmark = pytest.mark.gpu
F32, NU, NI = np.float32, 90, 517


def matrix_trainer(U, W, bias, t=None):
    t = t or new_trainer(len(U), len(W), U.shape[1])
    for name, v in (("W_user", U), ("W_item", W), ("i_bias", bias)):
        t.set_view(name, v)
    t.set_knob("rank_topn_scores", 1)
    return t


def model(nu, ni, k, seed, integer=True):
    """integer: entries in [-3, 3], biases in [-8, 8] (every order exact in fp32); else random normal"""
    rng = np.random.default_rng(seed)
    if integer:
        return rng.integers(-3, 4, (nu, k)).astype(F32), rng.integers(-3, 4, (ni, k)).astype(F32), rng.integers(-8, 9, ni).astype(F32)
    return rng.standard_normal((nu, k)).astype(F32), rng.standard_normal((ni, k)).astype(F32), rng.standard_normal(ni).astype(F32)


def allowed(S, ni, ban_ptr, ban_item):
    on = np.ones((S, ni), bool)
    on[np.repeat(np.arange(S), np.diff(ban_ptr)), ban_item.astype(np.int64)] = False
    return on


def plain_topn(score, on, top_n):
    """the rule on a [S][ni] score matrix: unbanned items by (-score, id)"""
    S, ni = score.shape
    items, scores, count = np.full((S, top_n), -1, np.int32), np.zeros((S, top_n), F32), on.sum(1).clip(max=top_n).astype(np.int32)
    for s in range(S):
        ids = np.flatnonzero(on[s])
        best = ids[np.lexsort((ids, -score[s, ids]))][:top_n]
        items[s, :len(best)], scores[s, :len(best)] = best, score[s, best]
    return items, scores, count, np.zeros(S, np.int32)


def assert_bounded(got, rows, W, bias, on, top_n, k):
    """the contract: every listed score within 2 (k + 2) 2^-24 (|b| + sum |u v|) of the float64 score of its id; key order; no banned id, no
    duplicate; the count; no unlisted candidate better than the worst listed one by more than both bounds"""
    items, scores, count, nan = got
    r64, W64, b64 = rows.astype(np.float64), W.astype(np.float64), bias.astype(np.float64)
    ref = b64[None, :] + r64 @ W64.T
    bound = 2.0 * (k + 2) * 2.0 ** -24 * (np.abs(b64)[None, :] + np.abs(r64) @ np.abs(W64).T)
    assert (count == on.sum(1).clip(max=top_n)).all() and not nan.any()
    worst = 0.0
    for s in range(len(rows)):
        ids, sc, bits = items[s, :count[s]].astype(np.int64), scores[s, :count[s]].astype(np.float64), scores[s, :count[s]].view(np.uint32)
        assert (items[s, count[s]:] == -1).all() and on[s, ids].all() and len(np.unique(ids)) == len(ids)
        worst = max(worst, float((np.abs(sc - ref[s, ids]) / bound[s, ids]).max(initial=0.0)))
        assert ((sc[:-1] > sc[1:]) | ((bits[:-1] == bits[1:]) & (ids[:-1] < ids[1:]))).all()
        rest = on[s] & ~np.isin(np.arange(len(W)), ids)
        if rest.any():
            last = ids[np.argmin(ref[s, ids])]
            assert (ref[s, rest] - ref[s, last] <= bound[s, rest] + bound[s, last]).all()
    print("largest |error| / bound at k = %d: %.4f" % (k, worst))
    assert worst <= 1.0
    return worst


CASES = [(k, S, NI) for k in (1, 3, 4, 33, 64, 130, 256, 257, 1024) for S in (1, 65, 203)] + [(64, 65, 129)]


@pytest.mark.parametrize("k, S, ni", CASES, ids=["k%d-S%d-ni%d" % c for c in CASES])
def test_integer_models_are_exact(k, S, ni):
    """every product and partial sum is exact in fp32 in any order, so ids and score bits equal int64 numpy and the pinned sweep's; the
    scores tie massively; chunk edges, tails, both sides of 256 floats, ragged section and item tiles, section 30 bans all but five items"""
    top_n = (1, 10, 256)[CASES.index((k, S, ni)) % 3]
    U, W, bias = model(NU, ni, k, seed=k + S)
    users, ban_ptr, ban_item = make_bans(S, NU, ni, seed=k)
    t = matrix_trainer(U, W, bias)
    got = t.rank_topn(users, top_n, ban_ptr, ban_item)
    score = bias.astype(np.int64)[None, :] + U[users].astype(np.int64) @ W.astype(np.int64).T
    assert_same(got, plain_topn(score, allowed(S, ni, ban_ptr, ban_item), top_n))
    t.set_knob("rank_topn_scores", 0)
    assert_same(got, t.rank_topn(users, top_n, ban_ptr, ban_item))


@pytest.mark.parametrize("k, top_n", [(7, 10), (64, 256), (130, 1), (320, 10)])
def test_float_models_keep_the_bound(k, top_n):
    S = 203
    U, W, bias = model(NU, NI, k, seed=k, integer=False)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k)
    got = matrix_trainer(U, W, bias).rank_topn(users, top_n, ban_ptr, ban_item)
    assert_bounded(got, U[users], W, bias, allowed(S, NI, ban_ptr, ban_item), top_n, k)


@pytest.mark.parametrize("k", [64, 320])
def test_edges_and_determinism(k):
    S, top_n, NAN, INF = 70, 10, 100, 200
    U, W, bias = model(NU, NI, k, seed=k, integer=False)
    U = np.abs(U) + F32(0.1)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k)
    users[[0, 37, 64]] = 5                        # one user at three places of the section tiles, with one ban list
    ban = [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    ban[37] = ban[64] = ban[0]
    ban = [np.concatenate([b, [NAN]]).astype(np.uint32) if 10 <= s < 20 else b[b != NAN] for s, b in enumerate(ban)]
    ban_ptr, ban_item = ptr_of(ban), np.concatenate(ban)
    on = allowed(S, NI, ban_ptr, ban_item)
    call = lambda: t.rank_topn(users, top_n, ban_ptr, ban_item)
    with_row = lambda i, v: (t.set_view("W_item", np.where(np.arange(NI)[:, None] == i, F32(v), W)), call())[1]
    t = new_trainer(NU, NI, k)
    matrix_trainer(U, W, bias, t).set_knob("rank_topn_scores", 0)
    pinned = call()
    t.set_knob("rank_topn_scores", 1)
    before = t.counter(50), t.counter(39)
    got = call()
    assert (t.counter(50) - before[0], t.counter(39) - before[1]) == (S, S)
    for s in (37, 64):
        assert_same([x[s] for x in got], [x[0] for x in got])
    t.set_knob("rank_topn_budget", 5 * t.rank_geometry("topn", S, top_n)["cap"])      # several pieces
    assert_same(call(), got)
    t.set_knob("rank_topn_budget", 1 << 25)
    first = with_row(INF, np.inf)                 # the user rows are positive: its score is +inf
    assert not first[3].any() and (first[0][on[:, INF], 0] == INF).all() and np.isposinf(first[1][on[:, INF], 0]).all() and (first[0][~on[:, INF]] != INF).all()
    flagged = with_row(NAN, np.nan)               # flags exactly the sections that do not ban it
    np.testing.assert_array_equal(flagged[3], on[:, NAN].astype(np.int32))
    np.testing.assert_array_equal(flagged[2], np.where(on[:, NAN], 0, got[2]))
    t.set_view("W_item", W)
    t.set_knob("rank_topn_scores", 0)
    assert_same(call(), pinned)                   # the mode leaves nothing behind


@pytest.mark.parametrize("route", ["fb", "lines", "dot", "cosine"])
def test_routes(route, tmp_path):
    k, S, top_n = 64, 70, 10
    U, W, bias = model(NU, NI, k, seed=len(route))
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=4)
    rng = np.random.default_rng(5)
    ptr = np.arange(0, 3 * S + 1, 3, dtype=np.int64)                      # three integer-valued entries per section
    val = rng.integers(-2, 3, 3 * S).astype(F32)
    if route in ("fb", "lines"):
        path = tmp_path / "feat_item.txt"                                  # even items carry one child, the odd id behind them, valued 2
        path.write_text("".join("1 %d:2\n" % (i + 1) if i % 2 == 0 and i + 1 < NI else "0\n" for i in range(NI)))
        t = sa.Trainer(int(route == "fb"), 0)
        for kk, v in fb_conf(NU, NI, k) if route == "fb" else lines_conf(NU, NI, k, 0, [("feature_item", str(path))]):
            t.set_param(kk, v)
        t.init_model(); t.init_trainer()
    if route == "fb":
        Wfb, idx = rng.integers(-3, 4, (NFB, k)).astype(F32), rng.integers(0, NFB, 3 * S).astype(np.uint32)
        t.set_view("W_ufeedback", Wfb)
        got = matrix_trainer(U, W, bias, t).rank_topn(users, top_n, ban_ptr, ban_item, feedback=(ptr, idx, val))
        rows = (Wfb[idx] * val[:, None]).reshape(S, 3, k).sum(1) + U[users]
    elif route == "lines":
        idx = rng.integers(0, NU, 3 * S).astype(np.uint32)
        got = matrix_trainer(U, W, bias, t).rank_topn(None, top_n, ban_ptr, ban_item, lines=(ptr, idx, val))
        rows = (U[idx] * val[:, None]).reshape(S, 3, k).sum(1)
        even = np.arange(0, NI - 1, 2)
        W[even] += 2 * W[even + 1]
        bias[even] += 2 * bias[even + 1]
    else:
        t = matrix_trainer(U, W, bias)
        got = t.similar_items(users, top_n, route, ban_ptr, ban_item)
        ban = [np.concatenate([ban_item[a:b], [q]]).astype(np.uint32) for q, a, b in zip(users, ban_ptr[:-1], ban_ptr[1:])]
        ban_ptr, ban_item, bias = ptr_of(ban), np.concatenate(ban), np.zeros(NI, F32)
        W = sa.item_unit_rows(W) if route == "cosine" else W
        rows = W[users]
    on = allowed(S, NI, ban_ptr, ban_item)
    if route == "cosine":
        assert_bounded(got, rows, W, bias, on, top_n, k)
    else:
        assert_same(got, plain_topn(bias.astype(np.int64)[None, :] + rows.astype(np.int64) @ W.astype(np.int64).T, on, top_n))

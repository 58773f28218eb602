"""Deep top-N lists (knob rank_topn_deep = 1, top_n 257 .. 4096) on the GPU in both scoring modes, against numpy: integer models
(every summation order exact, massive ties) scored in int64 and ordered by (-score, id) -- ids, score bits, counts and flags must be equal."""
import numpy as np
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from test_gpu_rank_matrix import allowed, assert_bounded, matrix_trainer, model, plain_topn
from test_gpu_rank_topn import assert_same, make_bans, pressure_model, ptr_of
from test_rank_feedback import NFB, fb_conf
from test_rank_lines import lines_conf

pytestmark = pytest.mark.gpu
F32, NU, NI = np.float32, 90, 5000
MODES = {"pinned": 0, "matrix": 1}


def deep_trainer(U, W, bias, mode, t=None):
    t = matrix_trainer(U, W, bias, t)
    t.set_knob("rank_topn_scores", MODES[mode])
    t.set_knob("rank_topn_deep", 1)
    return t


def ranges(t, S, top_n, gy=3):
    """rank_topn_budget set to gy lists per section: one piece of S sections over gy item ranges, asserted through the probe"""
    cap = -(-2 * top_n // 128) * 128
    t.set_knob("rank_topn_budget", gy * cap * S)
    g = t.rank_geometry("topn", S, top_n)
    assert (g["gy"], g["sections"], g["cap"]) == (gy, S, cap)
    return g


def int_lists(U, W, bias, users, ban_ptr, ban_item, top_n):
    score = bias.astype(np.int64)[None, :] + U[users].astype(np.int64) @ W.astype(np.int64).T
    return plain_topn(score, allowed(len(users), len(W), ban_ptr, ban_item), top_n)


@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("k", [3, 64, 130, 257])          # two candidates per lane (3, 64), one (130), the wide sweep (257)
@pytest.mark.parametrize("mode", list(MODES))
def test_integer_models_are_exact(mode, k, S):
    """5000 items in three ranges; of 65 sections one bans a whole range, one the first range, one all but 40 items (a short list, padding).
    A range of about 1 700 items fills no list of top_n 1 000 / 4 096: there only the merge selects; the sweeps' cut runs at 257, and below"""
    U, W, bias = model(NU, NI, k, seed=k + S)
    t = deep_trainer(U, W, bias, mode)
    t.set_knob("rank_topn_prefilter", 1)                   # no effect on a deep call: the counters 51 / 52 do not move
    per = ranges(t, S, 257)["items_per_block"]
    users, ban_ptr, ban_item = rg.geometry_bans(S, NU, NI, per, 3, seed=k)
    want = int_lists(U, W, bias, users, ban_ptr, ban_item, 4096)
    before = np.array([t.counter(c) for c in (61, 39, 50, 51, 52)])
    for n in (257, 1000, 4096):
        assert ranges(t, S, n)["items_per_block"] == per
        assert_same(t.rank_topn(users, n, ban_ptr, ban_item), rg.cut_lists(want, n))
    assert (np.array([t.counter(c) for c in (61, 39, 50, 51, 52)]) - before).tolist() == [3 * S, 3 * S, 3 * S * MODES[mode], 0, 0]


@pytest.mark.parametrize("top_n", [257, 4096])
@pytest.mark.parametrize("mode, k", [("pinned", 8), ("pinned", 130), ("pinned", 260), ("matrix", 8)])
def test_an_increasing_model_cuts_every_list(mode, k, top_n):
    """score strictly ascending in the id: every step appends, every top_n appends force a cut; a range of 15 000 items cuts at least twice"""
    nu, ni, S = 30, 30000, 5
    U, W, bias = pressure_model("increasing", nu, ni, k, None)
    t = deep_trainer(U, W, bias, mode)
    g = ranges(t, S, top_n, gy=2)
    assert g["items_per_block"] > g["cap"] + top_n
    users, ban_ptr, ban_item = make_bans(S, nu, ni, seed=top_n)
    assert_same(t.rank_topn(users, top_n, ban_ptr, ban_item), int_lists(U, W, bias, users, ban_ptr, ban_item, top_n))


def test_a_float_model():
    """pinned: the first 256 of a list of 1000 are the knob-0 list of 256, bit for bit -- seed 6 is chosen so that in every section the
    float64 scores of ranks 256 and 257 lie further apart than twice the matrix bound (checked here on the CPU); matrix: section 6ah's contract"""
    k, S, n = 64, 20, 1000
    U, W, bias = model(NU, NI, k, seed=6, integer=False)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k)
    on = allowed(S, NI, ban_ptr, ban_item)
    r64, W64, b64 = U[users].astype(np.float64), W.astype(np.float64), bias.astype(np.float64)
    top = -np.sort(-np.where(on, b64[None, :] + r64 @ W64.T, -np.inf), 1)
    bound = 2.0 * (k + 2) * 2.0 ** -24 * (np.abs(b64)[None, :] + np.abs(r64) @ np.abs(W64).T)
    assert (top[:, 255] - top[:, 256] > 2 * bound.max(1)).all()
    t = deep_trainer(U, W, bias, "pinned")
    ranges(t, S, n)
    deep = t.rank_topn(users, n, ban_ptr, ban_item)
    t.set_knob("rank_topn_deep", 0)
    flat = t.rank_topn(users, 256, ban_ptr, ban_item)
    np.testing.assert_array_equal(deep[0][:, :256], flat[0])
    np.testing.assert_array_equal(deep[1][:, :256].view(np.uint32), flat[1].view(np.uint32))
    assert (deep[2] == n).all() and not deep[3].any()
    deep_trainer(U, W, bias, "matrix", t)
    assert_bounded(t.rank_topn(users, n, ban_ptr, ban_item), U[users], W, bias, on, n, k)


@pytest.mark.parametrize("mode", list(MODES))
def test_edges(mode):
    """num_item = top_n + 1; a NaN row among the ranked candidates; top_n <= 256 under the knob is the knob-0 call and counts nothing"""
    k, S, ni, NAN = 64, 70, 258, 100
    U, W, bias = model(NU, ni, k, seed=1)
    users, ban_ptr, ban_item = make_bans(S, NU, ni, seed=2)
    t = deep_trainer(U, W, bias, mode)
    assert_same(t.rank_topn(users, 257, ban_ptr, ban_item), int_lists(U, W, bias, users, ban_ptr, ban_item, 257))
    before = [t.counter(c) for c in (61, 51, 52)]
    got = t.rank_topn(users, 100, ban_ptr, ban_item)
    assert [t.counter(c) for c in (61, 51, 52)] == before
    t.set_knob("rank_topn_deep", 0)
    assert_same(got, t.rank_topn(users, 100, ban_ptr, ban_item))
    t.set_knob("rank_topn_deep", 1)
    t.set_view("W_item", np.where(np.arange(ni)[:, None] == NAN, F32(np.nan), W))
    items, scores, count, nan = t.rank_topn(users, 257, ban_ptr, ban_item)
    on = allowed(S, ni, ban_ptr, ban_item)
    np.testing.assert_array_equal(nan, on[:, NAN].astype(np.int32))
    np.testing.assert_array_equal(count, np.where(on[:, NAN], 0, on.sum(1).clip(max=257)))
    assert (items[nan == 1] == -1).all() and (scores[nan == 1] == 0).all()


@pytest.mark.parametrize("route", ["fb", "lines", "cosine"])
def test_routes(route):
    """top_n 300 through _fb and _lines (pinned, exact) and similar_items (cosine: the matrix mode, within its bound)"""
    k, S, top_n, ni = 64, 70, 300, 517
    U, W, bias = model(NU, ni, k, seed=len(route))
    users, ban_ptr, ban_item = make_bans(S, NU, ni, seed=4)
    if route == "cosine":
        t = deep_trainer(U, W, bias, "matrix")
        got = t.similar_items(users, top_n, route, ban_ptr, ban_item)
        ban = [np.concatenate([ban_item[a:b], [q]]).astype(np.uint32) for q, a, b in zip(users, ban_ptr[:-1], ban_ptr[1:])]
        unit = sa.item_unit_rows(W)
        assert_bounded(got, unit[users], unit, np.zeros(ni, F32), allowed(S, ni, ptr_of(ban), np.concatenate(ban)), top_n, k)
        assert t.counter(61) == S and t.counter(49) == S
        return
    rng = np.random.default_rng(5)
    ptr, val = np.arange(0, 3 * S + 1, 3, dtype=np.int64), rng.integers(-2, 3, 3 * S).astype(F32)   # three integer-valued entries per section
    src = rng.integers(-3, 4, (NFB, k)).astype(F32) if route == "fb" else U
    idx = rng.integers(0, len(src), 3 * S).astype(np.uint32)
    t = sa.Trainer(int(route == "fb"), 0)
    for kk, v in fb_conf(NU, ni, k) if route == "fb" else lines_conf(NU, ni, k, 0):
        t.set_param(kk, v)
    t.init_model(); t.init_trainer()
    deep_trainer(U, W, bias, "pinned", t)
    if route == "fb":
        t.set_view("W_ufeedback", src)
    got = t.rank_topn(users if route == "fb" else None, top_n, ban_ptr, ban_item, **{"feedback" if route == "fb" else "lines": (ptr, idx, val)})
    rows = (src[idx] * val[:, None]).reshape(S, 3, k).sum(1) + (U[users] if route == "fb" else 0)
    assert_same(got, plain_topn(bias.astype(np.int64)[None, :] + rows.astype(np.int64) @ W.astype(np.int64).T, allowed(S, ni, ban_ptr, ban_item), top_n))
    assert t.counter(61) == S

"""Rank positions through the certified counting sweep on the matrix cores (knob rank_eval_prefilter = 1, svdf_k_rankeval_mfma.hip; DESIGN.md
6aj) on the GPU: position, tied, ranked and nan are the knob-0 call's of the same trainer -- and the numpy statement of the documented rule's
-- whether a section is certified (counter 53) or ranked again by the pinned sweep (counter 54)."""
import numpy as np
import pytest

import svdfeature_amd as sa
from rank_rounding import cluster, score_fp32
from test_gpu_rank_eval import make_sections, new_trainer, ranked_count, rule_positions
from test_gpu_rank_matrix import model
from test_gpu_rank_prefilter import relisted_pieces_case, relisted_rule_rows
from test_rank_feedback import NFB, fb_conf, rule_pos
from test_rank_lines import lines_conf

pytestmark = pytest.mark.gpu
F32, NU, NI = np.float32, 90, 517
KS = (3, 33, 64, 130, 257, 1024)
# mixed needs both routes, so more than one section; and at k = 3 cluster(.., 400) has no section with more than 64 items within
# (k + 2) 2^-24 H_s = 5 ulp of a positive (0 of 70 in float64: three entries moved by up to 400 ulp each spread the scores over hundreds)
CASES = [(kind, k, S) for kind in ("float", "integer") for k in KS for S in (1, 70)] + [("mixed", k, 70) for k in KS[1:]]


def trainer_of(U, W, bias, t=None):
    t = t or new_trainer(len(U), len(W), U.shape[1])
    for name, v in (("W_user", U), ("W_item", W), ("i_bias", bias)):
        t.set_view(name, v)
    return t


def both(t, call, pos_ptr):
    """the call with the knob at 0 and at 1: all four outputs equal; returns the knob-1 result and how far the counters 53 / 54 moved"""
    t.set_knob("rank_eval_prefilter", 0)
    want = call()
    t.set_knob("rank_eval_prefilter", 1)
    before = [t.counter(c) for c in (53, 54, 38)]
    got = call()
    moved = [t.counter(c) - b for c, b in zip((53, 54, 38), before)]
    n = int((np.diff(pos_ptr) > 0).sum())
    print("certified %d, ranked again %d of %d" % (moved[0], moved[1], n))
    assert moved[0] + moved[1] == n and moved[2] == n
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    return got, moved[:2]


def assert_rule(got, score, lists):
    """the documented rule on a [section][item] score matrix"""
    users, pos_ptr, pos_item, ban_ptr, ban_item = lists
    for s in range(len(users)):
        a, b = pos_ptr[s], pos_ptr[s + 1]
        position, tied = rule_positions(score[s], pos_item[a:b].astype(np.int64), ban_item[ban_ptr[s]:ban_ptr[s + 1]].astype(np.int64))
        assert (got[0][a:b].tolist(), got[1][a:b].tolist()) == (position, tied)
    np.testing.assert_array_equal(got[2], ranked_count(score.shape[1], ban_ptr, ban_item))


@pytest.mark.parametrize("kind, k, S", CASES, ids=["%s-k%d-S%d" % c for c in CASES])
def test_the_positions_are_the_pinned_positions(kind, k, S):
    U, W, bias = model(NU, NI, k, seed=k + S, integer=kind == "integer")
    lists = make_sections(S, NU, NI, seed=k)
    if kind == "mixed":   # even items: a cluster a few hundred ulp wide; one positive per section, an even item in even sections; no bans
        rng = np.random.default_rng(k)
        W[::2], bias = cluster(rng, NI, k, 400)[::2], np.zeros(NI, F32)
        pos = (2 * rng.integers(0, NI // 2, S) + np.arange(S) % 2).astype(np.uint32)
        lists = (lists[0], np.arange(S + 1, dtype=np.int64), pos, np.zeros(S + 1, np.int64), np.zeros(0, np.uint32))
    users, pos_ptr, pos_item = lists[:3]
    t = trainer_of(U, W, bias)
    t.set_knob("rank_eval_prefilter_band", 64 if kind == "mixed" else 1024)
    got, moved = both(t, lambda: t.rank_positions(*lists), pos_ptr)
    if kind == "integer":
        assert_rule(got, bias.astype(np.int64)[None, :] + U[users].astype(np.int64) @ W.astype(np.int64).T, lists)
    elif k <= 300:
        assert_rule(got, np.stack([score_fp32(U[u], W, bias) for u in users]), lists)
    if kind == "float":
        assert moved[1] == 0   # 517 ids cannot overflow 1 024: the inputs alone certify every section
    if kind == "mixed":
        # float64, from the reference alone.  More than 64 items (the positive among them) closer to the positive than (k + 2) 2^-24 H_s lie
        # in its band whatever the rounding: the list overflows.  Fewer than 64 within 3 Delta_s -- 2 Delta_s between a band member's pinned
        # score and the positive's, Delta_s / 2 for the two pinned scores against float64, the outward rounding of lo / hi -- cannot.
        U64, W64 = U[users].astype(np.float64), W.astype(np.float64)
        H = np.abs(U64) @ np.abs(W64).max(0)
        s64 = U64 @ W64.T
        gap = np.abs(s64 - s64[np.arange(S), pos_item.astype(np.int64)][:, None])
        over = ((gap < ((k + 2) * 2.0 ** -24 * H)[:, None]).sum(1) > 64).sum()
        under = ((gap <= (12.0 * (k + 2) * 2.0 ** -24 * H + 3.0 * (k + 2) * 2.0 ** -124)[:, None]).sum(1) < 64).sum()
        assert over > 0 and under > 0 and moved[1] >= over and moved[0] >= under


@pytest.mark.parametrize("k", [64, 320])
def test_the_conditions_on_the_inputs(k):
    S, ROW = 70, 100
    U, W, bias = model(NU, NI, k, seed=k, integer=False)
    lists = make_sections(S, NU, NI, seed=k)
    users, pos_ptr = lists[0], lists[1]
    n, has = S - 1, np.diff(pos_ptr) > 0
    t = trainer_of(U, W, bias)
    call = lambda: t.rank_positions(*lists)
    put = lambda a, i, j, v: np.where((np.arange(len(a))[:, None] == i) & ((np.arange(k)[None, :] == j) | (j < 0)), F32(v), a)
    assert both(t, call, pos_ptr)[1] == [n, 0]
    t.set_view("W_item", put(W, 3, k - 1, 1e-40))
    assert both(t, call, pos_ptr)[1] == [0, n]            # a denormal on the item side: no section is certified
    t.set_view("W_item", W)
    t.set_view("W_user", put(U, 7, 0, 1e-40))
    assert both(t, call, pos_ptr)[1][1] == ((users == 7) & has).sum()   # ... in a user's row: its sections
    t.set_view("W_user", put(U, 7, 1, 2.0 ** 100))
    t.set_view("W_item", put(W, 3, 1, 2.0 ** 100))
    assert both(t, call, pos_ptr)[1][1] == ((users == 7) & has).sum()   # H_s > 2^126: only user 7 meets both 2^100 entries
    t.set_view("W_user", U)
    t.set_view("W_item", put(W, ROW, -1, np.inf))
    assert both(t, call, pos_ptr)[1] == [0, n]
    t.set_view("W_item", put(W, ROW, -1, np.nan))
    got, moved = both(t, call, pos_ptr)                    # the flags and the -1 positions are the pinned call's
    assert moved == [0, n] and got[3].any() and (got[0][np.repeat(got[3], np.diff(pos_ptr)) != 0] == -1).all()


def test_item_ranges_tiles_and_pieces():
    k, ni, S = 8, 2177, 71                                 # three ranges of 768 items, the last one ragged (641)
    U, W, bias = model(NU, ni, k, seed=1, integer=False)
    users, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(S - 1, NU, ni, seed=2)
    edges = np.array([0, 127, 128, 767, 768, 1535, 1536, 2176], np.uint32)   # first / last item of a tile, of a range, of the catalogue
    lists = (np.append(users, 5).astype(np.uint32), np.append(pos_ptr, pos_ptr[-1] + len(edges)), np.concatenate([pos_item, edges]),
             np.append(ban_ptr, ban_ptr[-1]), ban_item)
    t = trainer_of(U, W, bias)
    t.set_knob("rank_eval_prefilter", 1)
    g = t.rank_geometry("positions", S, pos_ptr=lists[1])
    assert g["gy"] >= 3 and g["items_per_block"] == 768 and g["sections"] == S
    got, moved = both(t, lambda: t.rank_positions(*lists), lists[1])
    assert moved == [S - 1, 0]
    assert_rule(got, np.stack([score_fp32(U[u], W, bias) for u in lists[0]]), lists)
    t.set_knob("rank_eval_budget", 40 * 1026)              # two pieces: a row costs its band list of 1 024 ids and two words
    assert S // 3 < t.rank_geometry("positions", S, pos_ptr=lists[1])["sections"] < S
    for a, b in zip(both(t, lambda: t.rank_positions(*lists), lists[1])[0], got):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("k", [12, 300])
@pytest.mark.parametrize("rows", ["fb", "lines", "fb+lines"])
def test_relisted_sections_of_several_pieces(rows, k):
    """seven sections (tests/test_gpu_rank_prefilter.py: ragged lists, an empty one at the start and at the end, three sections that cannot
    be certified) in at least three pieces: the positions of the numpy rule and the outputs of the one-piece call with the knob at 0 --
    the offsets of a second piece and of the relisted subset are what is on trial"""
    S = 7
    t, users, kw, hot, m = relisted_pieces_case(rows, k)
    _, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(S, NU, NI, seed=k, big=2, empty=5, full_ban=-1, npos_big=40)
    call = lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item, **kw)
    t.set_knob("rank_eval_prefilter", 0)
    want = call()
    position, tied = rule_pos(relisted_rule_rows(users, kw, m), m[1], m[2], pos_ptr, pos_item, ban_ptr, ban_item)   # the numpy rule
    np.testing.assert_array_equal(want[0], position)
    np.testing.assert_array_equal(want[1], tied)
    np.testing.assert_array_equal(want[2], ranked_count(NI, ban_ptr, ban_item))
    assert not want[3].any()
    # a row of up to 28 positives costs its band list and two words, 1 026; a section adds at most 5 positives, 40 bans, 12 list entries and
    # 1: two sections with positives fit a piece, three do not -- sections 0 - 1, the two rows of section 2, 3 - 5, 6
    t.set_knob("rank_eval_budget", 2 * 1026 + 200)
    t.set_knob("rank_eval_prefilter", 1)
    assert t.rank_geometry("positions", S, pos_ptr=pos_ptr)["sections"] == 2
    got, moved = both(t, call, pos_ptr)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert moved == [S - 1 - len(hot), len(hot)]           # section 5 has no positives
    t.set_knob("rank_eval_budget", 1026)                   # section 2 alone exceeds the budget: ranked by the pinned route at once
    got, moved = both(t, call, pos_ptr)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    assert moved == [S - 2 - len(hot), len(hot) + 1]


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integer"])
@pytest.mark.parametrize("route", ["fb", "lines"])
def test_routes(route, integer, tmp_path):
    """a feature_item table; items 200 .. 399 are copies of one row, so a section with a positive among them has 200 candidates in its band
    and, at a capacity of 64, is ranked again from the gathered copies of its positives, ban list, feedback list and USER line"""
    k, S = 64, 70
    U, W, bias = model(NU, NI, k, seed=len(route), integer=integer)
    W[200:400], bias[200:400] = W[200], bias[200]
    lists = make_sections(S, NU, NI, seed=4)
    rng = np.random.default_rng(5)
    ptr = np.arange(0, 3 * S + 1, 3, dtype=np.int64)       # three entries per section
    val = rng.integers(-2, 3, 3 * S).astype(F32) if integer else rng.standard_normal(3 * S).astype(F32)
    path = tmp_path / "feat_item.txt"                      # items 400 .. carry one child, the id behind them, valued 2
    path.write_text("".join("1 %d:2\n" % (i + 1) if i >= 400 and i % 2 == 0 and i + 1 < NI else "0\n" for i in range(NI)))
    t = sa.Trainer(int(route == "fb"), 0)
    for kk, v in fb_conf(NU, NI, k) if route == "fb" else lines_conf(NU, NI, k, 0, [("feature_item", str(path))]):
        t.set_param(kk, v)
    t.init_model(); t.init_trainer()
    trainer_of(U, W, bias, t)
    if route == "fb":
        t.set_view("W_ufeedback", rng.integers(-3, 4, (NFB, k)).astype(F32) if integer else rng.standard_normal((NFB, k)).astype(F32))
        extra = dict(feedback=(ptr, rng.integers(0, NFB, 3 * S).astype(np.uint32), val))
    else:
        lists, extra = (None,) + lists[1:], dict(lines=(ptr, rng.integers(0, NU, 3 * S).astype(np.uint32), val))
    t.set_knob("rank_eval_prefilter_band", 64)
    before = [t.counter(c) for c in (40, 41)]
    moved = both(t, lambda: t.rank_positions(*lists, **extra), lists[1])[1]
    assert moved[0] > 0 and moved[1] > 0
    assert sum(t.counter(c) - b for c, b in zip((40, 41), before)) == 2 * (S - 1)   # two calls, each section once
    m1 = t.rank_eval(*lists, **extra)
    t.set_knob("rank_eval_prefilter", 0)
    assert t.rank_eval(*lists, **extra) == m1

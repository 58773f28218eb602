"""The certified matrix-core prefilter of the top-N calls (knob rank_topn_prefilter = 1, svdf_k_ranktopn_exact.hip) on the
GPU: its lists are the pinned lists, bit for bit -- against the knob-0 call of the same trainer and the numpy statement of the pinned order
-- whether a section is certified (counter 51) or listed again by the pinned sweep (counter 52)."""
import numpy as np
import pytest

import svdfeature_amd as sa
from rank_rounding import cluster, score_fp32
from test_gpu_rank_eval import new_trainer
from test_gpu_rank_matrix import allowed, model, plain_topn
from test_gpu_rank_topn import assert_same, make_bans, ptr_of
from item_topn_rule import rule_similar
from test_rank_feedback import NFB, fb_conf, rule_lists, rule_user_rows
from test_rank_lines import lines_conf, rule_line_rows

pytestmark = pytest.mark.gpu
F32, NU, NI = np.float32, 90, 517
KS, TOPS = (3, 12, 33, 64, 130, 257, 300, 1024), (1, 10, 100, 256)
# (kind, k, S, top_n): every k with both plain kinds, every S and top_n with each; the mixed kind where the fallback must act
CASES = [(kind, k, 1 if (i + j) % 3 == 0 else 70, TOPS[(i + 2 * j) % 4]) for j, kind in enumerate(("float", "integer")) for i, k in enumerate(KS)]
CASES += [("mixed", 64, 70, 100), ("mixed", 300, 70, 100), ("mixed", 12, 1, 10), ("mixed", 1024, 70, 256)]


def trainer_of(U, W, bias, t=None):
    t = t or new_trainer(len(U), len(W), U.shape[1])
    for name, v in (("W_user", U), ("W_item", W), ("i_bias", bias)):
        t.set_view(name, v)
    return t


def both(t, call, S):
    """the call under the prefilter and with the knob at 0: equal; returns the prefilter's result and how far the counters 51 / 52 moved"""
    t.set_knob("rank_topn_prefilter", 0)
    want = call()
    t.set_knob("rank_topn_prefilter", 1)
    before = [t.counter(c) for c in (51, 52, 50)]
    got = call()
    moved = [t.counter(c) - b for c, b in zip((51, 52, 50), before)]
    print("certified %d, listed again %d of %d" % (moved[0], moved[1], S))
    assert moved[0] + moved[1] == S and moved[2] == 0
    assert_same(got, want)
    return got, moved[:2]


@pytest.mark.parametrize("kind, k, S, top_n", CASES, ids=["%s-k%d-S%d-n%d" % c for c in CASES])
def test_the_lists_are_the_pinned_lists(kind, k, S, top_n):
    U, W, bias = model(NU, NI, k, seed=k + S, integer=kind == "integer")
    if kind == "mixed":   # a cluster a few hundred ulp wide between normal rows: the approximate order inside it is wrong
        rng = np.random.default_rng(k)
        W, bias = cluster(rng, NI, k, 400), np.zeros(NI, F32)
        W[1::2] = rng.standard_normal((NI, k)).astype(F32)[1::2]
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k)
    t = trainer_of(U, W, bias)
    got, moved = both(t, lambda: t.rank_topn(users, top_n, ban_ptr, ban_item), S)
    on = allowed(S, NI, ban_ptr, ban_item)
    if k <= 300:
        assert_same(got, plain_topn(np.stack([score_fp32(U[u], W, bias) for u in users]), on, top_n))
    if kind == "integer":
        assert_same(got, plain_topn(bias.astype(np.int64)[None, :] + U[users].astype(np.int64) @ W.astype(np.int64).T, on, top_n))
    if kind == "float":
        assert moved[1] == 0          # the float64 reference alone certifies every section (the scores lie many Delta_s apart)
    if kind == "mixed" and S == 70 and top_n == 100:
        assert moved[0] > 0 and moved[1] > 0


@pytest.mark.parametrize("k", [64, 320])
def test_the_conditions_on_the_inputs(k):
    S, top_n, ROW = 70, 10, 100
    U, W, bias = model(NU, NI, k, seed=k, integer=False)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k)
    ban = [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    ban = [np.concatenate([b, [ROW]]).astype(np.uint32) if 10 <= s < 20 else b[b != ROW] for s, b in enumerate(ban)]   # ROW is banned by ten sections
    ban_ptr, ban_item = ptr_of(ban), np.concatenate(ban)
    t = trainer_of(U, W, bias)
    call = lambda: t.rank_topn(users, top_n, ban_ptr, ban_item)
    put = lambda a, i, j, v: np.where((np.arange(len(a))[:, None] == i) & ((np.arange(k)[None, :] == j) | (j < 0)), F32(v), a)
    assert both(t, call, S)[1] == [S, 0]          # section 30 ranks five items: certified by "every candidate listed"
    t.set_view("W_item", put(W, 3, k - 1, 1e-40))
    assert both(t, call, S)[1] == [0, S]          # a denormal on the item side: no section is certified
    t.set_view("W_item", W)
    t.set_view("W_user", put(U, 7, 0, 1e-40))
    assert both(t, call, S)[1][1] == (users == 7).sum()   # ... in a user's row: its sections
    t.set_view("W_user", put(U, 7, 1, 2.0 ** 100))
    t.set_view("W_item", put(W, 3, 1, 2.0 ** 100))
    assert both(t, call, S)[1][1] >= (users == 7).sum()   # H_s > 2^126
    t.set_view("W_user", U)
    t.set_view("W_item", put(W, ROW, -1, np.inf))
    assert both(t, call, S)[1] == [0, S]
    t.set_view("W_item", put(W, ROW, -1, np.nan))
    got, moved = both(t, call, S)                  # the flags are the pinned call's: the sections that do not ban the row
    assert moved == [0, S]
    np.testing.assert_array_equal(got[3], allowed(S, NI, ban_ptr, ban_item)[:, ROW].astype(np.int32))


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integer"])
@pytest.mark.parametrize("route", ["fb", "lines", "dot", "cosine"])
def test_routes(route, integer, tmp_path):
    """float models: sections are certified; integer models at slack 1: wherever the scores at the ranks top_n and top_n + 1 tie, the pinned
    sweep lists the section again, from the gathered copies of its ban list, feedback list and USER line"""
    k, S, top_n = 64, 70, 10
    U, W, bias = model(NU, NI, k, seed=len(route), integer=integer)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=4)
    rng = np.random.default_rng(5)
    ptr = np.arange(0, 3 * S + 1, 3, dtype=np.int64)                      # three entries per section
    val = rng.integers(-2, 3, 3 * S).astype(F32) if integer else rng.standard_normal(3 * S).astype(F32)
    if route in ("fb", "lines"):
        path = tmp_path / "feat_item.txt"                                  # even items carry one child, the odd id behind them, valued 2
        path.write_text("".join("1 %d:2\n" % (i + 1) if i % 2 == 0 and i + 1 < NI else "0\n" for i in range(NI)))
        t = sa.Trainer(int(route == "fb"), 0)
        for kk, v in fb_conf(NU, NI, k) if route == "fb" else lines_conf(NU, NI, k, 0, [("feature_item", str(path))]):
            t.set_param(kk, v)
        t.init_model(); t.init_trainer()
        trainer_of(U, W, bias, t)
    if route == "fb":
        t.set_view("W_ufeedback", rng.integers(-3, 4, (NFB, k)).astype(F32) if integer else rng.standard_normal((NFB, k)).astype(F32))
        idx = rng.integers(0, NFB, 3 * S).astype(np.uint32)
        call = lambda: t.rank_topn(users, top_n, ban_ptr, ban_item, feedback=(ptr, idx, val))
    elif route == "lines":
        idx = rng.integers(0, NU, 3 * S).astype(np.uint32)
        call = lambda: t.rank_topn(None, top_n, ban_ptr, ban_item, lines=(ptr, idx, val))
    else:
        t = trainer_of(U, W, bias)
        call = lambda: t.similar_items(users, top_n, route, ban_ptr, ban_item)
    t.set_knob("rank_topn_prefilter_slack", 1 if integer else 32)
    before = [t.counter(c) for c in (39, 49, 40, 41)]
    moved = both(t, call, S)[1]
    rose = [t.counter(c) - b for c, b in zip((39, 49, 40, 41), before)]
    assert rose[0] + rose[1] == 2 * S and rose[2] + rose[3] == (2 * S if route in ("fb", "lines") else 0)   # two calls, each section once
    assert moved[0 if not integer or route == "cosine" else 1] > 0


def relisted_pieces_case(rows, k, S=7, hot=(1, 3, 4)):
    """S sections on a float model whose rows come from ragged lists of 0 - 6 entries -- `rows`: "fb", "lines" or "fb+lines" -- with an
    empty list in section 0 (the start of the first piece) and in section S - 1 (the end of the call).  Column 0 of W_user and of
    W_ufeedback is zero but for the denormal U[5, 0]: the row of a section that brings user 5 (as its user, or with value 1 in its line)
    holds a denormal and is not certified (a condition on the inputs, tests above); the sections `hot` bring it, the others cannot.
    Returns (trainer, users or None, the keyword lists, hot, the model: U, W, bias, W_ufeedback)."""
    rng = np.random.default_rng(k + len(rows))
    U, W, bias = model(NU, NI, k, seed=k, integer=False)
    Wfb = rng.standard_normal((NFB, k)).astype(F32)
    U[:, 0], Wfb[:, 0] = 0, 0
    U[5, 0] = F32(1e-40)
    fmt = int("fb" in rows)
    t = sa.Trainer(fmt, 0)
    for kk, v in lines_conf(NU, NI, k, fmt):
        t.set_param(kk, v)
    t.init_model(); t.init_trainer()
    trainer_of(U, W, bias, t)
    if fmt:
        t.set_view("W_ufeedback", Wfb)

    def ragged(n_id, with_5):
        lists = []
        for s in range(S):
            ids = rng.integers(6, n_id, 0 if s in (0, S - 1) else int(rng.integers(1, 7)))   # never id 5 by chance
            if with_5 and s in hot:
                ids[len(ids) // 2] = 5
            lists.append(ids.astype(np.uint32))
        idx = np.concatenate(lists)
        return ptr_of(lists), idx, np.where(idx == 5, 1, rng.standard_normal(len(idx))).astype(F32)

    kw = {}
    if "fb" in rows:
        kw["feedback"] = ragged(NFB, False)
    if "lines" in rows:
        kw["lines"] = ragged(NU, True)
        return t, None, kw, hot, (U, W, bias, Wfb)
    users = rng.integers(6, NU, S).astype(np.uint32)
    users[list(hot)] = 5
    return t, users, kw, hot, (U, W, bias, Wfb)


def relisted_rule_rows(users, kw, model_):
    """the sections' effective user rows by the numpy rules of tests/test_rank_feedback.py and tests/test_rank_lines.py"""
    U, _, _, Wfb = model_
    if "lines" in kw:
        return rule_line_rows(U, kw["lines"], None, Wfb, kw.get("feedback"))
    return rule_user_rows(U, Wfb, users, *kw["feedback"])


def relisted_items_case(k, S=7, hot=(1, 3, 4)):
    """an integer item matrix for svdf_item_topn whose ties are known: the query items 0 .. S - 1 are e_0 (e_1 for the sections `hot`), the
    items 100 .. 119 are 50 e_1, every other item i is (i + 10) e_0 + c_i e_2.  A hot query scores the twenty items 50 (dot) or 1 (cosine)
    and the rest below: rank top_n ties with rank top_n + 1, so at slack 1 the section is listed again.  Any other query scores item i
    i + 10 under dot: no tie, certified."""
    W = np.zeros((NI, k), F32)
    W[:, 0], W[:, 2] = np.arange(NI) + 10, np.arange(NI) * 7 % 13 + 1
    W[100:120] = 0
    W[100:120, 1] = 50
    W[:S] = 0
    W[:S, 0] = 1
    W[list(hot)] = 0
    W[list(hot), 1] = 1
    return W, np.arange(S, dtype=np.uint32), hot


@pytest.mark.parametrize("k", [12, 300])
@pytest.mark.parametrize("rows", ["fb", "lines", "fb+lines", "dot", "cosine"])
def test_relisted_sections_of_several_pieces(rows, k):
    """seven sections in at least three pieces, some certified and some listed again from the gathered copies of what they bring -- their
    ragged lists, or (dot, cosine: svdf_item_topn) their query items: the lists of the numpy rule and of the one-piece call with the knob
    at 0; the offsets of a second piece and of the relisted subset are what is on trial"""
    S, top_n = 7, 10
    _, ban_ptr, ban_item = make_bans(S, NU, NI, seed=k, almost_all=-1)
    if rows in ("dot", "cosine"):
        W, users, hot = relisted_items_case(k)
        t = trainer_of(np.zeros((NU, k), F32), W, np.zeros(NI, F32))
        t.set_knob("rank_topn_prefilter_slack", 1)
        call = lambda: t.similar_items(users, top_n, rows, ban_ptr, ban_item)
        rule = rule_similar(W, users, top_n, rows, ban_ptr, ban_item)
    else:
        t, users, kw, hot, m = relisted_pieces_case(rows, k)
        call = lambda: t.rank_topn(users, top_n, ban_ptr, ban_item, **kw)
        rule = rule_lists(relisted_rule_rows(users, kw, m), m[1], m[2], top_n, ban_ptr, ban_item)
    t.set_knob("rank_topn_prefilter", 0)
    want = call()
    assert_same(want, rule)
    t.set_knob("rank_topn_prefilter", 1)
    t.set_knob("rank_topn_budget", 3 * t.rank_geometry("topn", S, top_n)["cap"])    # three lists a piece
    assert t.rank_geometry("topn", S, top_n)["sections"] == 3
    got, moved = both(t, call, S)
    assert_same(got, want)
    if rows == "cosine":    # the hot sections by their ties; the others' unit scores may lie within Delta_s of each other
        assert moved[1] >= len(hot)
    else:
        assert moved == [S - len(hot), len(hot)]
    t.set_knob("rank_eval_budget", 6)                                               # ... and cut once more by the entries of the lists
    assert_same(both(t, call, S)[0], want)


def test_item_ranges_and_pieces():
    k, ni, S, top_n = 64, 3585, 70, 100
    U, W, bias = model(NU, ni, k, seed=1, integer=False)
    rng = np.random.default_rng(2)
    bias = np.zeros(ni, F32)
    W = cluster(rng, ni, k, 400)                                    # a cluster with a normal row at every twelfth place: sections are
    W[::12] = rng.standard_normal((ni, k)).astype(F32)[::12]        # certified or not by where the cluster ranks, over every range
    users, ban_ptr, ban_item = make_bans(S, NU, ni, seed=2)
    t = trainer_of(U, W, bias)
    t.set_knob("rank_topn_prefilter", 1)
    assert t.rank_geometry("topn", S, top_n)["gy"] >= 3
    got, moved = both(t, lambda: t.rank_topn(users, top_n, ban_ptr, ban_item), S)
    assert moved[0] > 0 and moved[1] > 0
    t.set_knob("rank_topn_budget", 5 * t.rank_geometry("topn", S, top_n)["cap"])
    assert t.rank_geometry("topn", S, top_n)["sections"] == 5      # fourteen pieces
    assert_same(both(t, lambda: t.rank_topn(users, top_n, ban_ptr, ban_item), S)[0], got)


def test_the_slack_changes_no_answer():
    k, S, top_n = 64, 70, 10
    U, W, bias = model(NU, NI, k, seed=9, integer=False)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=9)
    t = trainer_of(U, W, bias)
    got = {}
    for slack in (32, 1, 128):
        t.set_knob("rank_topn_prefilter_slack", slack)
        got[slack] = both(t, lambda: t.rank_topn(users, top_n, ban_ptr, ban_item), S)
        assert_same(got[slack][0], got[32][0])
    assert got[1][1][1] >= got[32][1][1]


def test_precedence_and_cleanliness():
    k, S, top_n = 64, 70, 10
    U, W, bias = model(NU, NI, k, seed=11, integer=False)
    users, ban_ptr, ban_item = make_bans(S, NU, NI, seed=11)
    t = trainer_of(U, W, bias)
    call = lambda: t.rank_topn(users, top_n, ban_ptr, ban_item)
    pinned = call()
    t.set_knob("rank_topn_scores", 1)
    matrix = call()
    t.set_knob("rank_topn_prefilter", 1)
    before = [t.counter(c) for c in (50, 51, 52)]
    assert_same(call(), matrix)                    # rank_topn_scores = 1 decides: the 6ah lists, exactly
    assert [t.counter(c) - b for c, b in zip((50, 51, 52), before)] == [S, 0, 0]
    t.set_knob("rank_topn_scores", 0)
    assert_same(call(), pinned)
    t.set_knob("rank_topn_prefilter", 0)
    assert_same(call(), pinned)                    # the mode leaves nothing behind

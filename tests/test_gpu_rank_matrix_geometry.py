"""The selecting sweep on the matrix cores (knob rank_topn_scores = 1, svdf_k_ranktopn_mfma.hip) over the launch geometries the
real workload reaches, on the GPU: item splits over 3, 7, 8 and 14 workgroups in y with ragged, full and one-item last ranges at row widths
on either side of every route of the pinned sweeps; the top_n values at which a list's capacity, sort size and threshold slot change, on a
model that cuts at every tile; a NaN row that is a whole range; `similar_items`, `_fb` and `_lines` over several ranges; and the sentence
"the bits of a score are a function of its two rows, the bias and k alone", across grids, positions and pieces, bit for bit.  Integer
models are compared with int64 numpy exactly, float models with float64 under the published bound and nothing else.  Every case asserts
through the probe svdf_rank_geometry that the handle under test has the geometry the case is about.  The shapes, lists and models come
from tests/rank_matrix_cases.py (and through it tests/rank_geometry.py); tests/test_rank_matrix_cases.py proves their properties."""
import numpy as np
import pytest

import rank_geometry as rg
import rank_matrix_cases as mc
import svdfeature_amd as sa
import test_gpu_rank_feedback as fbt
import test_gpu_rank_lines as lnt
from test_gpu_rank_eval import new_trainer
from test_gpu_rank_matrix import allowed, assert_bounded, model, plain_topn
from test_gpu_rank_topn import assert_same
from test_rank_feedback import rule_user_rows
from test_rank_lines import rule_item_side, rule_line_rows

pytestmark = pytest.mark.gpu
F32, NS, NU = np.float32, mc.NS, mc.NU

_scratch = {}


def scratch(name, ni=None, k=None):
    """one handle per geometry (or per (items, width) of the grid test) for the models written with set_view; every test sets its own"""
    if name not in _scratch:
        c = mc.inputs(name) if ni is None else dict(ni=ni, k=k)
        _scratch[name] = new_trainer(NU, c["ni"], c["k"])
    return _scratch[name]


def set_model(t, U, W, bias, knob=1):
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", bias)
    t.set_knob("rank_topn_scores", knob)


def assert_geometry(t, c, tops, units=NS):
    """with the knob at 1 the handle splits the items as the case claims"""
    t.set_knob("rank_topn_scores", 1)
    k, ni, gy, last = mc.GEOMETRIES[c["name"]]
    for n in tops:
        g = t.rank_geometry("topn", units, n)
        assert (g["gy"], g["items_per_block"], ni - (gy - 1) * g["items_per_block"], g["cap"]) == (gy, c["per"], last, mc.matrix_cap(k, n)), n
        assert (g["sections"], g["tile_rows"]) == (units, 64)


def matrix_call(t, call):
    """a call under the knob at 1: the counters 50 and 39 (49 for an item call) rise by the sections"""
    t.set_knob("rank_topn_scores", 1)
    before = [t.counter(w) for w in (50, 39, 49)]
    got = call()
    rose = [t.counter(w) - b for w, b in zip((50, 39, 49), before)]
    assert rose[0] == len(got[2]) and rose[1] + rose[2] == len(got[2]), rose
    return got


def pinned_call(t, call):
    t.set_knob("rank_topn_scores", 0)
    before = t.counter(50)
    try:
        got = call()
    finally:
        t.set_knob("rank_topn_scores", 1)
    assert t.counter(50) == before
    return got


def assert_same_but_zeros(got, pinned):
    """6ah promises nothing about the sign of a zero score: the pinned sweep is compared on the sections whose pinned list holds none"""
    keep = ~mc.holds_zero(pinned)
    assert_same([x[keep] for x in got], [x[keep] for x in pinned])
    np.testing.assert_array_equal(got[0], pinned[0])             # (the ids, counts and flags of every section)
    np.testing.assert_array_equal(got[2], pinned[2])
    return int(keep.sum())


def bounded(label, *args):
    worst = assert_bounded(*args)
    print("matrix geometry: %s: largest |error| / bound %.4f" % (label, worst))


@pytest.mark.parametrize("case", rg.MODELS)
@pytest.mark.parametrize("name", mc.NAMES)
def test_integer_models_over_every_item_split(name, case):
    """the pressure models of test_gpu_rank_topn and the two of rank_geometry (one winner per range, with top_n = gy and gy + 1 too; ties
    across every range boundary, a +-0 pair among them) on ban lists that empty a middle range, the first range, and leave 40 items over
    the ranges.  Every score is exact in fp32 in any order: ids, score bits, counts and flags equal int64 numpy, whose zeros are +0, and
    the pinned sweep wherever it lists no zero"""
    c = mc.inputs(name)
    want, score, (U, W, bias) = mc.want_lists(name, case)
    t = scratch(name)
    set_model(t, U, W, bias)
    tops = mc.tops_of(case, c["gy"])
    assert_geometry(t, c, tops)
    lists = (c["ban_ptr"], c["ban_item"])
    compared = 0
    for n in tops:
        got = matrix_call(t, lambda: t.rank_topn(c["users"], n, *lists))
        assert_same(got, rg.cut_lists(want, n))
        assert not (np.signbit(got[1]) & (got[1] == 0)).any()
        compared += assert_same_but_zeros(got, pinned_call(t, lambda: t.rank_topn(c["users"], n, *lists)))
    assert compared >= NS                                        # (of the len(tops) x 70 lists; the CPU test counts them per model)


@pytest.mark.parametrize("case", ["increasing", "float"])
@pytest.mark.parametrize("name", mc.CUT_GEOMETRIES)
def test_the_cut_points_of_the_lists(name, case):
    """top_n on either side of 64, 128, 192 and 256: min(cnt, top_n), the threshold buf[top_n - 1], the sort over the next power of two and
    the capacity (256 or 512; doubled or at the ceiling) change between them.  Under the increasing model every candidate beats the
    threshold, so every tile appends and a full range cuts its list again and again (tests/test_rank_matrix_cases.py states how often);
    a seeded random normal model goes through the bound"""
    c = mc.inputs(name)
    t = scratch(name)
    assert_geometry(t, c, rg.CUT_TOPS)
    lists = (c["ban_ptr"], c["ban_item"])
    if case == "increasing":
        want, score, (U, W, bias) = mc.want_lists(name, case)
    else:
        U, W, bias = mc.float_model(NU, c["ni"], c["k"], seed=c["k"])
        on = allowed(NS, c["ni"], *lists)
    set_model(t, U, W, bias)
    assert len({(mc.matrix_cap(c["k"], n), rg.cap_regime(mc.mk(c["k"]), n)) for n in rg.CUT_TOPS}) >= 2
    for n in rg.CUT_TOPS:
        got = matrix_call(t, lambda: t.rank_topn(c["users"], n, *lists))
        if case == "increasing":
            assert_same(got, rg.cut_lists(want, n))
        else:
            bounded("cut points %s top_n %d" % (name, n), got, U[c["users"]], W, bias, on, n, c["k"])


@pytest.mark.parametrize("name", mc.ONE_ITEM_LAST)
def test_a_nan_row_that_is_the_whole_last_range(name):
    """the single item of the one-item last range turns NaN; even sections ban it, odd sections rank it (a few of either already did the
    other).  The flags are exactly the ranking sections, whose lists are empty; the banning sections are what they were before, bit for bit"""
    c = mc.inputs(name)
    ni, t, n = c["ni"], scratch(name), 100
    U, W, bias = mc.float_model(NU, ni, c["k"], seed=c["k"] + 1)
    ban = []
    for s in range(NS):
        b = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]]
        ban.append(np.concatenate([b, [ni - 1]]).astype(np.uint32) if s % 2 == 0 else b)
    ban_ptr, ban_item = rg.ptr_of(ban), np.concatenate(ban)
    flags = np.array([0 if ni - 1 in b else 1 for b in ban], np.int32)
    assert 20 <= flags.sum() <= 40
    assert_geometry(t, c, (n,))
    assert ni - (c["gy"] - 1) * c["per"] == 1
    set_model(t, U, W, bias)
    clean = matrix_call(t, lambda: t.rank_topn(c["users"], n, ban_ptr, ban_item))
    bounded("before the NaN row %s" % name, clean, U[c["users"]], W, bias, allowed(NS, ni, ban_ptr, ban_item), n, c["k"])
    bad = W.copy()
    bad[ni - 1] = np.nan
    t.set_view("W_item", bad)
    got = matrix_call(t, lambda: t.rank_topn(c["users"], n, ban_ptr, ban_item))
    np.testing.assert_array_equal(got[3], flags)
    assert (got[2][flags == 1] == 0).all() and (got[0][flags == 1] == -1).all() and (got[1][flags == 1] == 0).all()
    assert_same([x[flags == 0] for x in got], [x[flags == 0] for x in clean])


@pytest.mark.parametrize("k", mc.GRID_KS)
def test_scores_do_not_depend_on_the_grid(k):
    """517 item rows and biases ranked on a trainer of their own (one range) and as the first, then as the LAST 517 rows of a catalogue of
    2 113 (three ranges; every section bans the rest, whose rows are other random floats): the same lists, the same score bits, the ids
    moved by a constant.  At the end of the large catalogue the rows lie in other ranges, other tiles and, 1 596 = 12 x 128 + 60, at other
    places of their tiles"""
    small, large, shift = mc.GRID_SMALL, mc.GRID_LARGE, mc.GRID_LARGE - mc.GRID_SMALL
    U, W, bias = mc.float_model(NU, small, k, seed=k)
    _, other_w, other_b = mc.float_model(NU, large, k, seed=k + 1)
    users, ban_ptr, ban_item = mc.grid_bans(seed=k)
    ts, tl = scratch(("grid", small, k), small, k), scratch(("grid", large, k), large, k)
    set_model(ts, U, W, bias)
    for n in (10, 256):
        assert ts.rank_geometry("topn", NS, n)["gy"] == 1
        base = matrix_call(ts, lambda: ts.rank_topn(users, n, ban_ptr, ban_item))
        bounded("grid k %d top_n %d" % (k, n), base, U[users], W, bias, allowed(NS, small, ban_ptr, ban_item), n, k)
        for at, lo, hi in ((0, small, large), (shift, 0, shift)):
            Wl, bl = other_w.copy(), other_b.copy()
            Wl[at:at + small], bl[at:at + small] = W, bias
            set_model(tl, U, Wl, bl)
            g = tl.rank_geometry("topn", NS, n)
            assert (g["gy"], g["items_per_block"]) == (3, 768)
            p, b = mc.shifted_bans(ban_ptr, ban_item, at, lo, hi)
            got = matrix_call(tl, lambda: tl.rank_topn(users, n, p, b))
            assert_same(got, (np.where(base[0] >= 0, base[0] + at, -1), base[1], base[2], base[3]))


@pytest.mark.parametrize("name", ["k8-gy3-ragged", "k1024-gy3-ragged"])
def test_scores_do_not_depend_on_the_position(name):
    """one item row and bias planted at five ids -- the first, two at tile positions 16 b + 15 in the ranges 1 and 2, the first id of the
    ragged last tile and the last item --, each section banning all but one of them.  The row scores above every other for every user (the
    user rows are positive), so every section lists its copy first, and its score has the same bits in every section of the same user --
    user 5 sits at the sections 0, 17, 37 and 64 with four different copies"""
    c = mc.inputs(name)
    k, ni, n = c["k"], c["ni"], 10
    U, W, bias = mc.float_model(NU, ni, k, seed=k + 2)
    U = np.abs(U) + F32(0.1)
    rng = np.random.default_rng(k)
    copies = mc.planted_ids(c)
    W[copies], bias[copies] = 3 * (np.abs(rng.standard_normal(k)) + 1).astype(F32), F32(0.37)
    users, ban_ptr, ban_item, kept = mc.planted_sections(c)
    on = allowed(NS, ni, ban_ptr, ban_item)
    ref = bias.astype(np.float64)[None, :] + U[users].astype(np.float64) @ W.astype(np.float64).T
    rest = np.where(on & ~np.isin(np.arange(ni), copies)[None, :], ref, -np.inf).max(1)
    assert (ref[np.arange(NS), kept] > 2 * rest).all() and (rest > 0).all()      # far above the bound of either score
    t = scratch(name)
    set_model(t, U, W, bias)
    assert_geometry(t, c, (n,))
    got = matrix_call(t, lambda: t.rank_topn(users, n, ban_ptr, ban_item))
    bounded("planted copies %s" % name, got, U[users], W, bias, on, n, k)
    np.testing.assert_array_equal(got[0][:, 0], kept)
    bits = got[1][:, 0].view(np.uint32)
    first = {int(u): int(bits[np.flatnonzero(users == u)[0]]) for u in np.unique(users)}
    np.testing.assert_array_equal(bits, np.array([first[int(u)] for u in users], np.uint32))
    at = list(mc.SAME_AT)
    assert len(set(kept[at].tolist())) == 4 and len(set(bits[at].tolist())) == 1


def test_scores_do_not_depend_on_the_pieces():
    """rank_topn_budget at 66 lists: pieces of 64 and 6 sections, the first held to ONE item range where the free split has 14, the second
    to 11; at 150 lists: one piece over two ranges.  Both are the single-piece call over 14 ranges, bit for bit"""
    name = "k8-gy14-ragged"
    c = mc.inputs(name)
    U, W, bias = mc.float_model(NU, c["ni"], c["k"], seed=14)
    t = scratch(name)
    set_model(t, U, W, bias)
    lists = (c["ban_ptr"], c["ban_item"])
    try:
        for n in (10, 256):
            assert_geometry(t, c, (n,))
            cap = mc.matrix_cap(c["k"], n)
            single = matrix_call(t, lambda: t.rank_topn(c["users"], n, *lists))
            bounded("pieces top_n %d" % n, single, U[c["users"]], W, bias, allowed(NS, c["ni"], *lists), n, c["k"])
            t.set_knob("rank_topn_budget", 66 * cap)
            g = t.rank_geometry("topn", NS, n)
            assert (g["sections"], g["gy"], g["items_per_block"]) == (64, 1, 106 * mc.TILE) and g["gy"] < c["gy"]
            g = t.rank_geometry("topn", NS - 64, n)              # the second piece
            assert (g["sections"], g["gy"], g["items_per_block"]) == (6, 11, 10 * mc.TILE)
            assert_same(matrix_call(t, lambda: t.rank_topn(c["users"], n, *lists)), single)
            t.set_knob("rank_topn_budget", 150 * cap)
            g = t.rank_geometry("topn", NS, n)
            assert (g["sections"], g["gy"], g["items_per_block"]) == (NS, 2, 53 * mc.TILE)
            assert_same(matrix_call(t, lambda: t.rank_topn(c["users"], n, *lists)), single)
            t.set_knob("rank_topn_budget", rg.TOPN_BUDGET)
    finally:
        t.set_knob("rank_topn_budget", rg.TOPN_BUDGET)


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_similar_items_over_seven_ranges(metric):
    """70 query items over every range -- id 0, the last id of range 0, the first of range 1 and the last item among them -- on the lists
    of the geometry (a range emptied in the middle, the first range emptied, 40 items left).  Dot on an integer model equals int64 numpy
    with bias 0 and the query appended to its bans, and the pinned sweep; cosine keeps the bound on sa.item_unit_rows; no query lists itself"""
    name = "k64-gy7-full"
    c = mc.inputs(name)
    k, ni, per = c["k"], c["ni"], c["per"]
    q = np.linspace(0, ni - 1, NS).astype(np.uint32)
    q[[1, 2]] = per - 1, per
    assert q[0] == 0 and q[-1] == ni - 1 and set((q // per).tolist()) == set(range(c["gy"]))
    ban = [np.concatenate([c["ban_item"][a:b], [x]]).astype(np.uint32) for x, a, b in zip(q, c["ban_ptr"][:-1], c["ban_ptr"][1:])]
    on = allowed(NS, ni, rg.ptr_of(ban), np.concatenate(ban))
    t = scratch(name)
    U, W, bias = model(NU, ni, k, seed=7) if metric == "dot" else mc.float_model(NU, ni, k, seed=7)
    set_model(t, U, W, bias)
    assert_geometry(t, c, (10, 256))
    for n in (10, 256):
        got = matrix_call(t, lambda: t.similar_items(q, n, metric, c["ban_ptr"], c["ban_item"]))
        assert not (got[0] == q.astype(np.int32)[:, None]).any()
        if metric == "dot":
            assert_same(got, plain_topn(W[q].astype(np.int64) @ W.astype(np.int64).T, on, n))
            assert_same_but_zeros(got, pinned_call(t, lambda: t.similar_items(q, n, metric, c["ban_ptr"], c["ban_item"])))
        else:
            unit = sa.item_unit_rows(W)
            bounded("cosine top_n %d" % n, got, unit[q], unit, np.zeros(ni, F32), on, n, k)


def check_trained_route(c, call, rows, W, bias, S, label):
    """a trained fixture of the pinned tests at 2 177 items under the knob at 1: three ranges, the bound against the float64 product of the
    rule's effective rows; and the knob back at 0, the pinned lists as they were"""
    t, n = c["t"], c["N"]
    try:
        t.set_knob("rank_topn_scores", 1)
        g = t.rank_geometry("topn", S, n)
        assert (g["gy"], g["items_per_block"], g["cap"]) == (3, 768, mc.matrix_cap(64, n))
        got = matrix_call(t, call)
        bounded(label, got, rows, W, bias, allowed(S, len(W), c["ban_ptr"], c["ban_item"]), n, 64)
    finally:
        t.set_knob("rank_topn_scores", 0)
    assert_same(call(), c["got"][0])


def test_feedback_sections_over_three_item_ranges():
    c = fbt.trained(64, 2177)
    rows = rule_user_rows(c["U"], c["Wfb"], c["users"], *c["fb"])
    check_trained_route(c, lambda: c["t"].rank_topn(c["users"], c["N"], c["ban_ptr"], c["ban_item"], feedback=c["fb"]), rows, c["W"], c["bias"], fbt.NS,
                        "feedback sections")


def test_lines_sections_with_both_tables_over_three_item_ranges(tmp_path_factory):
    c = lnt.trained(tmp_path_factory.mktemp("rank_matrix_lines"), 64, 0, "generated", 2177)
    assert c["table_u"] is not None and c["table_i"] is not None
    rows = rule_line_rows(c["U"], c["lines"], c.get("table_u"), c.get("Wfb"), c.get("fb"))
    W, bias = rule_item_side(c["W"], c["bias"], c.get("table_i"))
    check_trained_route(c, lambda: c["t"].rank_topn(None, c["N"], c["ban_ptr"], c["ban_item"], lines=c["lines"], feedback=c.get("fb")), rows, W, bias,
                        lnt.NS, "lines sections")

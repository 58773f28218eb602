"""The launch geometry of the live-model ranking calls, the parts that need no GPU: the probe svdf_rank_geometry -- the
functions the launches call, on a host-only handle -- against the Python statement of the rule in tests/rank_geometry.py; the geometries
tests/test_gpu_rank_geometry.py claims to reach; and the properties of that test's inputs, proved on the numpy rules alone."""
import numpy as np
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from rank_rounding import score_fp32
from test_gpu_rank_eval import rule_positions
from test_rank_topn import rule_topn

KS = (8, 64, 128, 132, 200, 256, 260, 320, 1024)
SECTIONS = (1, 64, 65, 5000, 200000)
TOPS = (1, 32, 33, 64, 65, 96, 97, 192, 193, 224, 225, 256)     # either side of every top_n at which the capacity or its regime changes
ITEMS = sorted(set(list(range(1, 300)) + [m * 64 + d for m in range(1, 20000 // 64 + 1) for d in (-1, 0, 1)] + [20000]))
BINDING = 1 << 14                                                # rank_topn_budget: 32 lists of 512 keys


def probe_handle(k, ni):
    """the probe needs the parameters only: no model is allocated, so a handle is cheap and may change its shape"""
    t = sa.Trainer(0, 0, 0, device=-2)
    shape(t, k, ni)
    return t


def shape(t, k, ni):
    t.set_param("num_factor", str(k))
    t.set_param("num_item", str(ni))


@pytest.mark.parametrize("k", KS)
def test_the_probe_equals_the_rule(k):
    """item counts 1 .. 299, every multiple of 64 (so of 128) up to 20 000 and its two neighbours; top-N and positions; the budget knob at
    its default and where it binds (fewer ranges first, then pieces of whole tiles)"""
    t = probe_handle(k, 1)
    assert ITEMS[-1] == 20000 and {127, 128, 129, 19967, 19968, 19969} <= set(ITEMS)
    bound = 0
    for ni in ITEMS:
        t.set_param("num_item", str(ni))
        for units in SECTIONS:
            assert t.rank_geometry("positions", units) == rg.eval_geometry(k, ni, units), (ni, units)
            for budget in (rg.TOPN_BUDGET, BINDING):
                t.set_knob("rank_topn_budget", budget)
                for n in TOPS if ni % 64 == 0 else (1, 100, 256):
                    got, want = t.rank_geometry("topn", units, n), rg.topn_geometry(k, ni, units, n, budget)
                    assert got == want, (ni, units, n, budget, got, want)
                    bound += budget == BINDING and got != rg.topn_geometry(k, ni, units, n)
    assert bound > 1000                                          # the lowered budget did change answers
    t.set_knob("rank_topn_budget", rg.TOPN_BUDGET)
    for ni in (1, 129, 3585, 20000):
        t.set_param("num_item", str(ni))
        for n in range(1, 257):
            assert t.rank_geometry("topn", 70, n) == rg.topn_geometry(k, ni, 70, n), (ni, n)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_geometry("topn", 70, 257)
    with pytest.raises(sa.SvdfError, match="bad arguments"):
        t.rank_geometry("topn", 0, 1)


@pytest.mark.parametrize("k", KS)
def test_the_capacity_rule(k):
    """a list holds top_n kept keys and one step's appends -- what bounds the sweep's append, `cnt + popc <= cap` -- and never more than a
    wave sorts.  The rule's `top_n + tile` arm never decides: the doubling stops at 2 top_n + tile or more.  So its regimes are three:
    128 as it starts, a doubled capacity, and the ceiling of 512 where the doubling would pass it"""
    ti = rg.item_tile(k)
    t = probe_handle(k, 5000)
    seen = set()
    for n in range(1, 257):
        cap = t.rank_geometry("topn", 70, n)["cap"]
        doubled = 128
        while doubled < 2 * n + ti:
            doubled *= 2
        assert cap == rg.topn_cap(k, n) == min(doubled, rg.SORT_KEYS) and n + ti <= cap <= rg.SORT_KEYS
        regime = rg.cap_regime(k, n)
        assert (regime == "start") == (doubled == 128) and (regime == "ceiling") == (doubled > rg.SORT_KEYS)
        seen.add(regime)
    assert seen == ({"doubled", "ceiling"} if ti == 128 else {"start", "doubled", "ceiling"})


def test_the_cut_points_reach_every_regime_of_the_capacity():
    reached = {}
    for name in rg.CUT_GEOMETRIES:
        k = rg.GEOMETRIES[name][0]
        for n in rg.CUT_TOPS + (1, 100, 256):
            reached.setdefault(rg.cap_regime(k, n), set()).add(rg.topn_cap(k, n))
    assert reached == {"start": {128}, "doubled": {256, 512}, "ceiling": {512}}
    # ... and on each sweep the capacity changes inside the cut points
    for name in rg.CUT_GEOMETRIES:
        k = rg.GEOMETRIES[name][0]
        assert len({rg.topn_cap(k, n) for n in rg.CUT_TOPS}) == 2 and len({rg.cap_regime(k, n) for n in rg.CUT_TOPS}) == 2


@pytest.mark.parametrize("name", list(rg.GEOMETRIES))
def test_the_named_geometries_are_what_the_probe_says(name):
    c = rg.geometry_inputs(name)
    k, ni, gy, last = rg.GEOMETRIES[name]
    t = probe_handle(k, ni)
    for n in (1, 100, 256, gy, gy + 1) + rg.CUT_TOPS:
        g = t.rank_geometry("topn", rg.NS, n)
        assert (g["gy"], g["items_per_block"], ni - (gy - 1) * g["items_per_block"]) == (gy, c["per"], last), n
        assert g["tiles"] == (rg.NS if rg.wide(k) else 2) and g["sections"] == rg.NS
    assert rg.item_count(k, rg.NS, gy, "full" if last == c["per"] else last) == ni          # the helper finds these very counts
    assert rg.item_tile(k) == (128 if k <= 128 else 64) and rg.wide(k) == (k > 256)
    assert (ni % rg.item_tile(k) == 0) == (name == "two-per-lane-gy7-full")
    # the positives: the evaluation sweep splits the items the same way (the wide one has no ranges), over more than one tile of rows
    g = t.rank_geometry("positions", rg.NS, pos_ptr=c["pos_ptr"])
    assert g == rg.eval_geometry(k, ni, pos_ptr=c["pos_ptr"])
    assert (g["gy"], g["items_per_block"]) == ((1, ni) if rg.wide(k) else (gy, c["per"]))
    assert g["rows"] == rg.NS + 1 and g["tiles"] >= 2 and g["sections"] == rg.NS
    npos = np.diff(c["pos_ptr"])
    assert npos[rg.BIG] == rg.NPOS_BIG > rg.TILE_POSITIVES and npos[rg.TIE_SECTION] == 2 * (gy - 1)
    for s in range(rg.NS):                                       # positives lie in every range that has a ranked item
        p = c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]]
        free = np.setdiff1d(np.arange(ni), c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]])
        if s != rg.TIE_SECTION:
            assert set(rg.range_of(p, c["per"]).tolist()) == set(rg.range_of(free, c["per"]).tolist()), s
        assert not np.isin(p, c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]]).any() and len(np.unique(p)) == len(p)


def test_the_geometries_cover_what_the_issue_names():
    gys = {g[2] for g in rg.GEOMETRIES.values()}
    assert gys == {3, 7, 8, 14}
    one = {(rg.item_tile(k), rg.wide(k)) for k, ni, gy, last in rg.GEOMETRIES.values() if last == 1}
    assert one == {(128, False), (64, False), (64, True)}        # a one-item last range on each of the three sweeps
    assert {rg.GEOMETRIES[n][2] >= 3 for n in rg.CUT_GEOMETRIES} == {True}
    assert {(rg.item_tile(rg.GEOMETRIES[n][0]), rg.wide(rg.GEOMETRIES[n][0])) for n in rg.CUT_GEOMETRIES} == one


def test_the_row_chunks_are_what_the_probe_says():
    """32 768 + 40 rows in one piece under the default budget: two launches of the wide sweep, the 600 positives of section STRADDLE on the
    last row of the first and the first row of the second"""
    t = probe_handle(rg.CH_K, rg.CH_NI)
    for nan_call in (False, True):
        users, pos_ptr, pos_item, ban_ptr, ban_item = rg.chunk_sections(nan_call)
        g = t.rank_geometry("positions", rg.CH_S, pos_ptr=pos_ptr)
        assert g == rg.eval_geometry(rg.CH_K, rg.CH_NI, pos_ptr=pos_ptr)
        assert (g["rows"], g["launches"], g["sections"], g["tile_rows"]) == (rg.CH_ROWS, 2, rg.CH_S, 1)
        assert pos_ptr[-1] + ban_ptr[-1] + rg.CH_S <= rg.EVAL_BUDGET          # with its bans too the call is one piece
        first_row = np.concatenate([[0], np.cumsum(-(-np.diff(pos_ptr) // rg.TILE_POSITIVES))])
        assert (first_row[rg.FIRST_BIG], first_row[rg.STRADDLE], first_row[rg.BEHIND]) == (0, rg.WIDE_ROWS - 1, rg.WIDE_ROWS + 1)
        assert first_row[rg.STRADDLE + 1] - first_row[rg.STRADDLE] == 2 and (np.diff(pos_ptr) >= 1).all()
        assert not (pos_item == rg.NAN_ITEM).any()
        for s in (0, 1, 777, rg.STRADDLE, rg.BEHIND, rg.CH_S - 1):
            assert not np.isin(pos_item[pos_ptr[s]:pos_ptr[s + 1]], ban_item[ban_ptr[s]:ban_ptr[s + 1]]).any()
        ranks_nan = [s for s in range(rg.CH_S) if rg.NAN_ITEM not in ban_item[ban_ptr[s]:ban_ptr[s + 1]]]
        assert nan_call == (ranks_nan == [rg.STRADDLE, rg.BEHIND])
    t.set_knob("rank_eval_budget", 1000)                         # (the probe does see the budget)
    assert t.rank_geometry("positions", rg.CH_S, pos_ptr=pos_ptr)["sections"] < rg.CH_S


_want = {}


def want_lists(name, case):
    """rule_topn at top_n = 256 on one geometry's lists under one integer model, and the model's exact scores; computed once"""
    if (name, case) not in _want:
        c = rg.geometry_inputs(name)
        U, W, bias = rg.model_for(case, c)
        _want[(name, case)] = rule_topn(U, W, bias, c["users"], 256, c["ban_ptr"], c["ban_item"]), rg.exact_scores(U, W, bias), (U, W, bias)
    return _want[(name, case)]


PROVED = ("two-per-lane-gy3", "two-per-lane-gy8-one", "wide-gy8-one")       # a geometry of every sweep; the others share the builders


@pytest.mark.parametrize("name", PROVED)
def test_the_inputs_have_the_properties_the_gpu_test_is_about(name):
    c = rg.geometry_inputs(name)
    ni, per, gy = c["ni"], c["per"], c["gy"]
    banned = [set(c["ban_item"][a:b].tolist()) for a, b in zip(c["ban_ptr"][:-1], c["ban_ptr"][1:])]
    # every integer model: the float64 product narrows to fp32 exactly and equals the pinned order; no score is -0 (0 + x never is)
    for case in rg.MODELS:
        _, (s32, exact), (U, W, bias) = want_lists(name, case)
        assert exact
        np.testing.assert_array_equal(score_fp32(U[3], W, bias).view(np.uint32), s32[3].view(np.uint32))
        assert not (np.signbit(s32) & (s32 == 0)).any()
    # one winner per range: with top_n = gy the list of a section that bans no winner is the winners, one from every range
    want, _, _ = want_lists(name, "winners")
    win = rg.winners_of(ni, per, gy)
    assert rg.range_of(win, per).tolist() == list(range(gy)) and win[0] == per - 1 and win[-1] == ni - 1
    clean = [s for s in range(rg.NS) if not banned[s] & set(win.tolist())]
    assert len(clean) >= 60
    for s in clean:
        assert sorted(rg.range_of(rg.cut_lists(want, gy)[0][s], per).tolist()) == list(range(gy))
        assert set(rg.cut_lists(want, gy + 1)[0][s, :gy].tolist()) == set(win.tolist())
    # boundary ties: the two ids lie in different ranges, score the same, and are adjacent in the list in id order -- the +-0 pair too
    want, (s32, _), (U, W, bias) = want_lists(name, "boundary")
    assert np.signbit(bias[per - 1]) and not np.signbit(bias[per]) and bias[per - 1] == bias[per] == 0
    checked = 0
    for s in range(rg.NS):
        for a, b in rg.boundary_pairs(ni, per, gy):
            assert b == a + 1 and a // per + 1 == b // per and s32[c["users"][s], a] == s32[c["users"][s], b]
            if not banned[s] & {a, b} and s != rg.FEW_LEFT:
                row = rg.cut_lists(want, 100)[0][s].tolist()
                assert row.index(b) == row.index(a) + 1, (s, a)
                checked += 1
    assert checked >= 60 * (gy - 1)
    # ... and the positives of TIE_SECTION tie across every boundary
    s = rg.TIE_SECTION
    p = c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]].astype(np.int64)
    position, tied = rule_positions(s32[c["users"][s]], p, np.array(sorted(banned[s]), np.int64))
    assert (np.array(tied) >= 1).all() and sorted(position) == list(range(len(p)))
    # bans: a middle range without a ranked item and a full list all the same; the first range emptied under the equal model: the list
    # starts at the second range's first id; fewer than top_n items left, in at least three ranges
    want, _, _ = want_lists(name, "equal")
    m = gy // 2
    assert 0 < m < gy - 1 and set(range(m * per, min((m + 1) * per, ni))) <= banned[rg.EMPTY_MIDDLE]
    assert want[2][rg.EMPTY_MIDDLE] == 256 and m not in rg.range_of(want[0][rg.EMPTY_MIDDLE], per)
    assert set(range(per)) == banned[rg.EMPTY_FIRST] and want[0][rg.EMPTY_FIRST].tolist() == list(range(per, per + 256))
    left = want[0][rg.FEW_LEFT, :want[2][rg.FEW_LEFT]]
    assert want[2][rg.FEW_LEFT] == rg.LEFT < 100 and len(set(rg.range_of(left, per).tolist())) >= 3 and ni - 1 in left
    assert (want[0][rg.FEW_LEFT, rg.LEFT:] == -1).all()
    # the pressure the models are named for
    want, _, _ = want_lists(name, "increasing")
    assert (rg.range_of(want[0][0, :100], per) == gy - 1).all() or last_is_short(c)      # every earlier list is dropped by the merge
    assert (rg.range_of(want_lists(name, "decreasing")[0][0][0, :100], per) == 0).all()       # only the first range's list survives


def last_is_short(c):
    return c["ni"] - (c["gy"] - 1) * c["per"] < 256


@pytest.mark.parametrize("name", PROVED)
def test_a_merge_of_the_first_two_ranges_only_differs_from_the_rule(name):
    """the decoy of a merge kernel that visits min(gy, 2) lists: the rule over ban lists that also ban everything behind the second range.
    On the increasing model every section differs; on the winners, where the list is one item per range, too; on the decreasing model,
    whose list lies in the first range, none does -- the existing two-range cases could not tell"""
    c = rg.geometry_inputs(name)
    assert c["gy"] >= 3
    dp, di = rg.only_first_ranges(c["ban_ptr"], c["ban_item"], c["ni"], c["per"])
    for case, differ in (("increasing", rg.NS), ("winners", rg.NS - 10), ("decreasing", 0)):
        want, _, (U, W, bias) = want_lists(name, case)
        decoy = rule_topn(U, W, bias, c["users"], 256, dp, di)
        for n in (1, c["gy"], 100, 256):
            if case == "decreasing" and n > 100:
                continue
            rows = (rg.cut_lists(want, n)[0] != rg.cut_lists(decoy, n)[0]).any(axis=1)
            rows[[rg.EMPTY_FIRST, rg.FEW_LEFT]] = differ > 0        # (sections whose bans reach past the first range on their own)
            if case == "winners" and n < c["gy"]:
                continue
            assert rows.sum() >= differ if differ else not rows.any(), (case, n, int(rows.sum()))


def test_a_shorter_list_is_a_prefix_of_a_longer_one():
    c = rg.geometry_inputs("two-per-lane-gy3")
    want, _, (U, W, bias) = want_lists("two-per-lane-gy3", "ties")
    for n in (1, 63, 100):
        for a, b in zip(rg.cut_lists(want, n), rule_topn(U, W, bias, c["users"], n, c["ban_ptr"], c["ban_item"])):
            np.testing.assert_array_equal(a, b)


def test_the_vectorised_position_rule_is_the_rule():
    """rank_geometry.rule_positions_rows, the reference of the row-chunk case, against test_gpu_rank_eval.rule_positions section by section,
    on the tie-rich model with a NaN row that some sections rank"""
    c = rg.geometry_inputs("two-per-lane-gy3")
    _, (s32, _), _ = want_lists("two-per-lane-gy3", "ties")
    s32 = s32.copy()
    free = np.setdiff1d(np.arange(c["ni"]), c["pos_item"])[0]
    s32[:, free] = np.nan
    position, tied, ranked, nan = rg.rule_positions_rows(s32, c["users"], c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"])
    flagged = 0
    for s in range(rg.NS):
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        ban = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]].astype(np.int64)
        assert ranked[s] == c["ni"] - len(np.unique(ban))
        if free in ban:
            wp, wt = rule_positions(s32[c["users"][s]], c["pos_item"][a:b].astype(np.int64), ban)
            assert nan[s] == 0 and position[a:b].tolist() == wp and tied[a:b].tolist() == wt
        else:
            flagged += 1
            assert nan[s] == 1 and (position[a:b] == -1).all() and (tied[a:b] == -1).all()
    assert 0 < flagged < rg.NS and (tied > 0).any()

"""The inputs of tests/test_gpu_rank_matrix_geometry.py, the parts that need no GPU: the geometries it claims to reach, asked
of the probe on a host-only handle with the knob rank_topn_scores at 1; and, on the numpy rules alone, that those inputs tell a wrong
selecting sweep from a right one -- every decoy of tests/rank_matrix_cases.py lists something else, the increasing model forces the cuts
the cut test is about, and the zero scores are where the comparison with the pinned sweep leaves them out."""
import numpy as np
import pytest

import rank_geometry as rg
import rank_matrix_cases as mc
from test_rank_geometry import probe_handle
from test_rank_matrix import matrix_geometry


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_named_geometries_are_what_the_probe_says(name):
    c = mc.inputs(name)
    k, ni, gy, last = mc.GEOMETRIES[name]
    t = probe_handle(k, ni)
    t.set_knob("rank_topn_scores", 1)
    for n in mc.TOPS + (gy, gy + 1) + rg.CUT_TOPS:
        g = t.rank_geometry("topn", mc.NS, n)
        assert g == matrix_geometry(k, ni, mc.NS, n), n
        assert (g["gy"], g["items_per_block"], ni - (gy - 1) * g["items_per_block"], g["cap"]) == (gy, c["per"], last, mc.matrix_cap(k, n)), n
        assert (g["tiles"], g["tile_rows"], g["sections"]) == (2, 64, mc.NS) and c["per"] % mc.TILE == 0
    if last in (1, c["per"]):                                    # the helper finds these very counts
        assert rg.item_count(mc.mk(k), mc.NS, gy, "full" if last == c["per"] else last) == ni
    else:                                                        # ragged: whole tiles and one of 65 items, and no smaller catalogue has them
        assert last % mc.TILE == 65 and ni - mc.tail_start(c) == 65
        first = min(n for n in range(1, ni) if matrix_geometry(k, n, mc.NS, 1)["gy"] == gy)
        assert ni - first == 64 + (mc.TILE if gy == 14 else 0)
    t.set_knob("rank_topn_scores", 0)
    if k > 128:                                                  # the pinned rule splits these catalogues otherwise
        assert t.rank_geometry("topn", mc.NS, 1)["items_per_block"] != c["per"]


def test_the_geometries_cover_what_the_issue_names():
    shapes = {(k, gy, "one" if last == 1 else ("full" if ni % mc.TILE == 0 else "ragged")) for k, ni, gy, last in mc.GEOMETRIES.values()}
    assert shapes == {(8, 3, "ragged"), (64, 7, "full"), (33, 8, "one"), (200, 8, "one"), (260, 8, "one"), (1024, 3, "ragged"), (8, 14, "ragged")}
    assert max(ni for _, ni, _, _ in mc.GEOMETRIES.values()) <= 14000 and mc.GEOMETRIES["k1024-gy3-ragged"][1] == min(ni for _, ni, _, _ in mc.GEOMETRIES.values())
    assert rg.topn_geometry(200, 3585, mc.NS, 1)["gy"] == 8 and matrix_geometry(200, 3585, mc.NS, 1)["gy"] == 4
    assert [mc.GEOMETRIES[n][0] for n in mc.CUT_GEOMETRIES] == [8, 200, 260] and [mc.GEOMETRIES[n][0] for n in mc.ONE_ITEM_LAST] == [33, 200, 260]


@pytest.mark.parametrize("name", mc.NAMES)
def test_every_decoy_lists_something_else(name):
    """for every model used on this geometry, at the top_n values the GPU test asks for: the reference differs from each decoy in at least
    one section -- but for the pairs rank_matrix_cases.blind names, which must then NOT differ (the reason stands there)"""
    c = mc.inputs(name)
    for case in rg.MODELS:
        want, score, _ = mc.want_lists(name, case)
        for decoy in mc.DECOYS:
            sees = False
            caps = sorted({mc.matrix_cap(c["k"], n) for n in mc.TOPS}) if decoy == "append-order" else [None]   # only that decoy depends on the capacity
            for cap in caps:
                tops = [n for n in mc.TOPS if cap in (None, mc.matrix_cap(c["k"], n))]
                other = mc.decoy_lists(decoy, c, score, max(tops))
                for n in tops:
                    a, b = rg.cut_lists(want, n), rg.cut_lists(other, n)
                    sees |= bool((a[0] != b[0]).any() or (a[2] != b[2]).any())
            assert sees == (not mc.blind(name, case, decoy)), (case, decoy)


def test_no_decoy_is_blind_everywhere():
    for decoy in mc.DECOYS:
        seen = [(n, m) for n in mc.NAMES for m in rg.MODELS if not mc.blind(n, m, decoy)]
        assert len(seen) >= 6, decoy
    assert not any(mc.blind(n, "ties", d) or mc.blind(n, "winners", d) or mc.blind(n, "boundary", d) for n in mc.NAMES for d in mc.DECOYS
                   if d != "tail-tile-dropped")


@pytest.mark.parametrize("name", mc.CUT_GEOMETRIES)
def test_the_increasing_model_forces_the_cuts(name):
    """appends of 128 into `cap` slots, cut to top_n when cnt + 128 > cap: a full range of items_per_block / 128 tiles, every candidate
    beating the threshold (the score rises with the id), cuts a list at least three times at top_n = 1 and at least once at every cut
    point -- by the arithmetic; and on the sections' own ban lists every list of a full range that is not emptied is cut, at top_n = 1
    at least twice, and at least 70 lists as often as the arithmetic says"""
    c = mc.inputs(name)
    ntile = c["per"] // mc.TILE
    want, score, _ = mc.want_lists(name, "increasing")
    assert (np.diff(score, axis=1) > 0).all()                    # strictly increasing with the id, for every section
    for n in (1,) + rg.CUT_TOPS:
        cap, least = mc.matrix_cap(c["k"], n), 3 if n == 1 else 1
        assert n + mc.TILE <= cap <= rg.SORT_KEYS
        assert mc.forced_cuts([mc.TILE] * ntile, cap, n) >= least, n
        often = 0
        for s in range(mc.NS):                                   # (a few bans in a tile can save a list one cut: 122 + 124 keys leave room for 10)
            if s == rg.FEW_LEFT:
                continue
            cuts = [mc.forced_cuts(a, cap, n) for a in (mc.tile_appends(c, s, y) for y in range(c["gy"] - 1)) if len(a) == ntile and sum(a)]
            assert len(cuts) >= c["gy"] - 2 and min(cuts) >= max(1, least - 1), (n, s, cuts)
            often += sum(x >= least for x in cuts)
        assert often >= mc.NS, n


def test_the_cut_points_meet_two_regimes_of_the_capacity():
    for name in mc.CUT_GEOMETRIES:
        k = mc.GEOMETRIES[name][0]
        assert {rg.cap_regime(mc.mk(k), n) for n in rg.CUT_TOPS} == {"doubled", "ceiling"}
        assert {mc.matrix_cap(k, n) for n in rg.CUT_TOPS} == {256, 512}


@pytest.mark.parametrize("name", mc.NAMES)
def test_zero_scores_are_where_the_pinned_comparison_leaves_them_out(name):
    """the GPU test compares with the pinned sweep only on sections whose list holds no zero score: under the models with zero scores
    ("ties": zero rows with biases +-0; "boundary": a -0 / +0 pair across the first range boundary) such sections exist, and sections whose
    list does hold a zero exist too"""
    c = mc.inputs(name)
    with_zero = without = 0
    for case in ("ties", "boundary"):
        want, score, (U, W, bias) = mc.want_lists(name, case)
        assert (np.signbit(bias) & (bias == 0)).any() and not (np.signbit(want[1]) & (want[1] == 0)).any()
        for n in mc.TOPS:
            z = mc.holds_zero(rg.cut_lists(want, n))
            with_zero, without = with_zero + int(z.sum()), without + int((~z).sum())
        if case == "boundary":                                   # the +-0 pair is listed behind the gy - 1 planted pairs wherever it is not banned
            a, b = rg.boundary_pairs(c["ni"], c["per"], c["gy"])[0]
            both = [s for s in range(mc.NS) if {a, b} <= set(want[0][s].tolist())]
            assert len(both) >= 60 and all(want[0][s].tolist().index(b) == want[0][s].tolist().index(a) + 1 for s in both)
            assert mc.holds_zero(want).sum() >= 60 and not mc.holds_zero(rg.cut_lists(want, 1)).any()
    assert with_zero >= 60 and without >= 60


def test_the_planted_copies_lie_where_the_issue_names():
    for name in ("k8-gy3-ragged", "k1024-gy3-ragged"):
        c = mc.inputs(name)
        ids = mc.planted_ids(c)
        per = c["per"]
        assert ids[0] == 0 and ids[4] == c["ni"] - 1 and sorted(set((ids // per).tolist())) == [0, 1, 2]
        assert [int(i % mc.TILE) for i in ids[1:3]] == [16 * 2 + 15, 16 * 5 + 15] and ids[3] % mc.TILE == 0 and c["ni"] - ids[3] == 65
        users, ban_ptr, ban_item, kept = mc.planted_sections(c)
        assert (users[list(mc.SAME_AT)] == mc.SAME_USER).all() and len(set(kept[list(mc.SAME_AT)].tolist())) == 4
        assert {s // 16 for s in mc.SAME_AT} == {0, 1, 2, 4} and {s % 16 // 4 for s in mc.SAME_AT} == {0, 1}   # waves of two workgroups, two lane groups
        for s in range(mc.NS):
            b = set(ban_item[ban_ptr[s]:ban_ptr[s + 1]].tolist())
            assert len(b & set(ids.tolist())) == 4 and int(kept[s]) not in b
        per_user = [len(set(kept[users == u].tolist())) for u in np.unique(users)]
        assert sum(n >= 2 for n in per_user) >= 10                # many users meet their copy at two places or more


def test_the_grid_inputs():
    """517 items are one range, 2 113 three, at every width of the grid test; the moved rows sit at other tile positions"""
    for k in mc.GRID_KS:
        assert matrix_geometry(k, mc.GRID_SMALL, mc.NS, 10)["gy"] == 1 and matrix_geometry(k, mc.GRID_LARGE, mc.NS, 256)["gy"] == 3
    assert (mc.GRID_LARGE - mc.GRID_SMALL) % mc.TILE == 60
    users, ban_ptr, ban_item = mc.grid_bans(1)
    p, b = mc.shifted_bans(ban_ptr, ban_item, 0, mc.GRID_SMALL, mc.GRID_LARGE)
    assert (np.diff(p) == np.diff(ban_ptr) + mc.GRID_LARGE - mc.GRID_SMALL).all() and b.max() == mc.GRID_LARGE - 1

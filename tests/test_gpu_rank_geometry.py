"""The live-model ranking calls over the launch geometries the real workload reaches on the GPU: item splits over 3, 7, 8
and 14 workgroups in y with ragged, full and one-item last ranges on each of the three sweeps; the top_n values at which a list's capacity
and cut change; the second launch of the wide evaluation sweep.  Every comparison is bit for bit against the numpy rules
(tests/test_rank_topn.py: rule_topn, tests/test_gpu_rank_eval.py: rule_positions, the row rules of the feedback and lines tests); every case
asserts through the probe svdf_rank_geometry that the handle under test has the geometry the case is about.  The shapes, lists and models
come from tests/rank_geometry.py; tests/test_rank_geometry.py proves their properties on the rules alone."""
import numpy as np
import pytest

import cases
import rank_geometry as rg
import svdfeature_amd as sa
import test_gpu_rank_feedback as fbt
import test_gpu_rank_lines as lnt
from rank_rounding import score_fp32
from test_gpu_rank_eval import new_trainer, rule_positions
from test_gpu_rank_topn import assert_same, model_of
from test_rank_lines import rule_both as lines_rule_both
from test_rank_topn import rule_topn

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(rg.GEOMETRIES)
AT = (1, 10, 100)


def set_model(t, U, W, bias):
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", bias)


_scratch, _trained = {}, {}


def scratch(name):
    """one handle per geometry for the models written with set_view; every test sets its own"""
    if name not in _scratch:
        c = rg.geometry_inputs(name)
        _scratch[name] = new_trainer(rg.NU, c["ni"], c["k"])
    return _scratch[name]


def trained(name):
    """the model of a geometry after one training pass, with its rule results; computed once and shared (nothing changes them)"""
    if name not in _trained:
        c = rg.geometry_inputs(name)
        t = new_trainer(rg.NU, c["ni"], c["k"])
        t.train_dataset(t.dataset_from_triples(*cases.planted_triples(4000, rg.NU, c["ni"], seed=c["gy"])))
        U, W, bias = model_of(t)
        _trained[name] = dict(t=t, U=U, W=W, bias=bias, want=rule_topn(U, W, bias, c["users"], 256, c["ban_ptr"], c["ban_item"]))
    return _trained[name]


def assert_geometry(t, c, tops):
    """the handle under test splits the items as the case claims, for the lists and for the positions"""
    k, ni, gy, last = rg.GEOMETRIES[c["name"]]
    for n in tops:
        g = t.rank_geometry("topn", rg.NS, n)
        assert (g["gy"], g["items_per_block"], ni - (gy - 1) * g["items_per_block"], g["cap"]) == (gy, c["per"], last, rg.topn_cap(k, n)), n
    g = t.rank_geometry("positions", rg.NS, pos_ptr=c["pos_ptr"])
    assert (g["gy"], g["sections"], g["rows"]) == (1 if rg.wide(k) else gy, rg.NS, rg.NS + 1) and g["tiles"] >= 2


def want_positions(U, W, bias, users, pos_ptr, pos_item, ban_ptr, ban_item):
    """(position, tied, ranked, nan) by rule_positions on the pinned-order scores, section by section"""
    position, tied, nan = [], [], np.zeros(len(users), np.int32)
    ranked = np.array([len(W) - len(np.unique(ban_item[a:b])) for a, b in zip(ban_ptr[:-1], ban_ptr[1:])], np.int32)
    for s, u in enumerate(users):
        sc = score_fp32(U[u], W, bias)
        p = pos_item[pos_ptr[s]:pos_ptr[s + 1]].astype(np.int64)
        ban = ban_item[ban_ptr[s]:ban_ptr[s + 1]].astype(np.int64)
        on = np.ones(len(W), bool)
        on[ban] = False
        if np.isnan(sc[on]).any():
            nan[s] = 1
            wp = wt = [-1] * len(p)
        else:
            wp, wt = rule_positions(sc, p, ban)
        position += wp
        tied += wt
    return np.array(position, np.int32), np.array(tied, np.int32), ranked, nan


def check_both_calls(t, c, U, W, bias, tops, want=None):
    """rank_topn at every top_n of `tops` and rank_positions / rank_eval on the lists of c against the rules"""
    assert_geometry(t, c, tops)
    lists = (c["users"], c["ban_ptr"], c["ban_item"])
    if want is None:
        want = rule_topn(U, W, bias, c["users"], 256, c["ban_ptr"], c["ban_item"])
    before = t.counter(39)
    for n in tops:
        assert_same(t.rank_topn(lists[0], n, lists[1], lists[2]), rg.cut_lists(want, n))
    assert t.counter(39) - before == rg.NS * len(tops)
    args = (c["users"], c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"])
    got = t.rank_positions(*args)
    for a, b in zip(got, want_positions(U, W, bias, *args)):
        np.testing.assert_array_equal(a, b)
    assert not got[3].any() and (got[0] >= 0).all()
    m = t.rank_eval(*args, at=AT)
    assert m == sa.rank_metrics(c["pos_ptr"], got[0], ranked=got[2], nan=got[3], at=AT) and m["ninst"] == rg.NS


@pytest.mark.parametrize("case", rg.MODELS)
@pytest.mark.parametrize("name", NAMES)
def test_integer_models_over_every_item_split(name, case):
    """the four pressure models of test_gpu_rank_topn -- increasing: every later range beats all earlier lists, the merge drops them;
    decreasing: only the first range's list survives; equal: the smallest unbanned ids; ties -- and the two of rank_geometry: one winner per
    range (with top_n = gy and gy + 1 too) and ties across every range boundary, a +-0 pair among them.  The ban lists empty a middle range,
    the first range, and leave 40 items over the ranges; the positives lie in every range, 600 of them in one section, a tied pair per
    boundary in another.  Every score is exact in fp32: the reference is the float64 product, narrowed exactly"""
    c = rg.geometry_inputs(name)
    U, W, bias = rg.model_for(case, c)
    s32, exact = rg.exact_scores(U, W, bias)
    assert exact
    np.testing.assert_array_equal(score_fp32(U[5], W, bias).view(np.uint32), s32[5].view(np.uint32))
    t = scratch(name)
    set_model(t, U, W, bias)
    tops = (1, 100, 256) + ((c["gy"], c["gy"] + 1) if case == "winners" else ())
    check_both_calls(t, c, U, W, bias, tops)


@pytest.mark.parametrize("name", NAMES)
def test_a_trained_model_over_every_item_split(name):
    c, m = rg.geometry_inputs(name), trained(name)
    check_both_calls(m["t"], c, m["U"], m["W"], m["bias"], (1, 100, 256), want=m["want"])


@pytest.mark.parametrize("name", [n for n in NAMES if rg.GEOMETRIES[n][3] == 1])
def test_a_nan_row_that_is_the_whole_last_range(name):
    """the single item of the one-item last range turns NaN: the sections that rank it are flagged and list nothing, the sections that ban
    it are what the rule says -- and what they were before"""
    c, m = rg.geometry_inputs(name), trained(name)
    ni, t = c["ni"], scratch(name)
    W = m["W"].copy()
    W[ni - 1] = np.nan
    set_model(t, m["U"], W, m["bias"])
    ban, pos = [], []
    for s in range(rg.NS):
        b = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]]
        p = c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]]
        if s % 2 == 0:
            b, p = np.concatenate([b, [ni - 1]]).astype(np.uint32), p[p != ni - 1]
        ban.append(b)
        pos.append(p)
    ban_ptr, ban_item, pos_ptr, pos_item = rg.ptr_of(ban), np.concatenate(ban), rg.ptr_of(pos), np.concatenate(pos)
    g = t.rank_geometry("topn", rg.NS, 100)
    assert ni - (g["gy"] - 1) * g["items_per_block"] == 1 and g["gy"] == c["gy"]
    want = rule_topn(m["U"], W, m["bias"], c["users"], 100, ban_ptr, ban_item)
    flags = np.array([0 if ni - 1 in b else 1 for b in ban], np.int32)
    assert 20 <= flags.sum() <= 40
    got = t.rank_topn(c["users"], 100, ban_ptr, ban_item)
    assert_same(got, want)
    np.testing.assert_array_equal(got[3], flags)
    assert (got[2][flags == 1] == 0).all() and (got[0][flags == 1] == -1).all()
    clean = m["t"].rank_topn(c["users"], 100, ban_ptr, ban_item)
    assert_same([x[flags == 0] for x in got], [x[flags == 0] for x in clean])
    position = t.rank_positions(c["users"], pos_ptr, pos_item, ban_ptr, ban_item)
    for a, b in zip(position, want_positions(m["U"], W, m["bias"], c["users"], pos_ptr, pos_item, ban_ptr, ban_item)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(position[3], flags)


@pytest.mark.parametrize("case", ["increasing", "trained"])
@pytest.mark.parametrize("name", rg.CUT_GEOMETRIES)
def test_the_cut_points_of_the_lists(name, case):
    """top_n on either side of 64, 128, 192 and 256: min(cnt, top_n), the threshold buf[top_n - 1], the sort over the next power of two and
    the capacity (256 or 512; doubled or at the ceiling) change between them; the increasing model cuts the most"""
    c = rg.geometry_inputs(name)
    if case == "trained":
        m = trained(name)
        t, U, W, bias, want = m["t"], m["U"], m["W"], m["bias"], m["want"]
    else:
        U, W, bias = rg.model_for(case, c)
        t, want = scratch(name), None
        set_model(t, U, W, bias)
        want = rule_topn(U, W, bias, c["users"], 256, c["ban_ptr"], c["ban_item"])
    caps = set()
    for n in rg.CUT_TOPS:
        g = t.rank_geometry("topn", rg.NS, n)
        assert g["gy"] == c["gy"] >= 3 and g["cap"] == rg.topn_cap(c["k"], n)
        caps.add((g["cap"], rg.cap_regime(c["k"], n)))
        assert_same(t.rank_topn(c["users"], n, c["ban_ptr"], c["ban_item"]), rg.cut_lists(want, n))
    assert len(caps) >= 2


@pytest.mark.parametrize("case", ["increasing", "trained"])
def test_the_cut_points_of_candidate_lists(case):
    """k_rank_cand_select shares the sort and its cut: one list of 1 200 ids and shorter ones at the same top_n values; the rule is
    rule_topn with everything but the candidates banned"""
    name = "two-per-lane-gy3"
    c = rg.geometry_inputs(name)
    if case == "trained":
        m = trained(name)
        t, U, W, bias = m["t"], m["U"], m["W"], m["bias"]
    else:
        U, W, bias = rg.model_for(case, c)
        t = scratch(name)
        set_model(t, U, W, bias)
    rng = np.random.default_rng(12)
    cand = [np.sort(rng.permutation(c["ni"])[:n]).astype(np.uint32) for n in (1200, 64, 65, 513, 300, 255)]
    users = c["users"][:len(cand)]
    rest = [np.setdiff1d(np.arange(c["ni"]), x).astype(np.uint32) for x in cand]
    want = rule_topn(U, W, bias, users, 256, rg.ptr_of(rest), np.concatenate(rest))
    for n in rg.CUT_TOPS:
        assert_same(t.rank_topn(users, n, candidates=(rg.ptr_of(cand), np.concatenate(cand))), rg.cut_lists(want, n))


def test_feedback_sections_over_three_item_ranges():
    """a trained user-group model with 2 177 items: test_gpu_rank_feedback's sections, lists and rule at gy = 3"""
    ni = rg.GEOMETRIES["two-per-lane-gy3"][1]
    c = fbt.trained(64, ni)
    g = c["t"].rank_geometry("topn", fbt.NS, c["N"])
    assert g["gy"] == 3 and g["tiles"] == 3 and c["t"].rank_geometry("positions", fbt.NS, pos_ptr=c["pos_ptr"])["gy"] == 3
    lists, (position, tied) = fbt.rule_both(c)
    assert_same(c["got"][0], lists)
    np.testing.assert_array_equal(c["got"][1][0], position)
    np.testing.assert_array_equal(c["got"][1][1], tied)
    assert not c["got"][0][3].any() and not c["got"][1][3].any()


def test_lines_sections_with_both_tables_over_three_item_ranges(tmp_path_factory):
    """a trained model with a feature_user and a feature_item table and 2 177 items: test_gpu_rank_lines' sections, lines and rule at gy = 3"""
    ni = rg.GEOMETRIES["two-per-lane-gy3"][1]
    c = lnt.trained(tmp_path_factory.mktemp("rank_geometry_lines"), 64, 0, "generated", ni)
    assert c["table_u"] is not None and c["table_i"] is not None
    g = c["t"].rank_geometry("topn", lnt.NS, c["N"])
    assert g["gy"] == 3 and c["t"].rank_geometry("positions", lnt.NS, pos_ptr=c["pos_ptr"])["gy"] == 3
    lists, (position, tied) = lines_rule_both(c, c["N"])
    assert_same(c["got"][0], lists)
    np.testing.assert_array_equal(c["got"][1][0], position)
    np.testing.assert_array_equal(c["got"][1][1], tied)
    assert not c["got"][0][3].any() and not c["got"][1][3].any()


_chunk = {}


def chunk_trainer():
    if not _chunk:
        U, W, bias = rg.chunk_model()
        s32, exact = rg.exact_scores(U, W, bias)
        assert exact
        np.testing.assert_array_equal(score_fp32(U[7], W, bias).view(np.uint32), s32[7].view(np.uint32))
        t = new_trainer(rg.CH_NU, rg.CH_NI, rg.CH_K)
        set_model(t, U, W, bias)
        _chunk.update(t=t, U=U, W=W, bias=bias, s32=s32)
    return _chunk


def test_the_second_launch_of_the_wide_sweep():
    """num_factor 260 and 32 768 + 40 rows in one call: the wide sweep runs twice, the second launch on shifted row arrays; the section
    with 600 positives has its two rows on either side of the cut.  Positions, `tied`, `ranked` and the flags equal the (vectorised) rule"""
    m = chunk_trainer()
    t = m["t"]
    args = rg.chunk_sections()
    g = t.rank_geometry("positions", rg.CH_S, pos_ptr=args[1])
    assert (g["rows"], g["launches"], g["sections"]) == (rg.CH_ROWS, 2, rg.CH_S)
    before = t.counter(38)
    got = t.rank_positions(*args)
    assert t.counter(38) - before == rg.CH_S
    want = rg.rule_positions_rows(m["s32"], *args)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert not got[3].any() and (got[1] > 0).mean() > 0.5 and (got[2] == rg.CH_NI - np.diff(args[3])).all()
    mt = t.rank_eval(*args, at=AT)
    assert mt == sa.rank_metrics(args[1], got[0], ranked=got[2], nan=got[3], at=AT) and mt["ninst"] == rg.CH_S


def test_a_nan_row_counts_once_on_either_side_of_the_row_cut():
    """one item row turns NaN; the section across the cut and the one behind it rank it, every other section bans it.  Only a section's
    FIRST row counts its NaNs -- the ban kernel takes one back per banning section -- so the flags are 1 on those two and 0 elsewhere only
    if the second launch reads its own rows' row_first"""
    m = chunk_trainer()
    t = m["t"]
    W = m["W"].copy()
    W[rg.NAN_ITEM] = np.nan
    t.set_view("W_item", W)
    args = rg.chunk_sections(nan_call=True)
    assert t.rank_geometry("positions", rg.CH_S, pos_ptr=args[1])["launches"] == 2
    s32 = m["s32"].copy()
    s32[:, rg.NAN_ITEM] = np.nan
    try:
        got = t.rank_positions(*args)
    finally:
        t.set_view("W_item", m["W"])
    flags = np.zeros(rg.CH_S, np.int32)
    flags[[rg.STRADDLE, rg.BEHIND]] = 1
    np.testing.assert_array_equal(got[3], flags)
    for a, b in zip(got, rg.rule_positions_rows(s32, *args)):
        np.testing.assert_array_equal(a, b)

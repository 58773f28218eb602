"""Live-model ranking over per-section candidate lists on the GPU (svdf_rank_*_cand, svdf_k_rankcand.hip).  Three checkers:
the existing calls given the complement of a section's set as bans (every output and the scores' bits must be equal), the numpy statement of
the rule in tests/test_rank_cand.py, and, for the agreement of the routes, the CPU ranker on the saved model fed every section as USER / POS /
BAN / PROCESS lines."""
import numpy as np
import pytest

import svdfeature_amd as sa
from oracle import oracle
from test_gpu_rank_eval import port_positions
from test_gpu_rank_feedback import TOPS
from test_gpu_rank_lines import lines_trainer
from test_gpu_rank_topn import assert_same
from test_rank_cand import (NI, NOPOS, NS, NU, ROUNDING_KS, ROUTE_K, ROUTE_N, complement, make_candidates, rounding_input, rounding_results,
                            rule_cand_positions, rule_cand_topn)
from test_rank_feedback import NFB, make_feedback, rule_user_rows
from test_rank_lines import make_lines, rule_item_side, rule_line_rows, training_input, write_tables
from rank_rounding import DOT_DECOYS

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = (38, 39, 40, 41, 42)
KS = (7, 16, 64, 128, 200, 320)      # the tail, 64 / 32 / 16 staged rows in a turn, and a wide row (one lane per pair)
KINDS = ("users", "feedback", "lines")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("rank_cand")


def section_args(c):
    """(users, keywords) naming the sections of c for any of the three methods"""
    if c["kind"] == "lines":
        return None, dict(lines=c["lines"], feedback=c.get("fb"))
    return c["users"], dict(feedback=c.get("fb"))


def cand_both(t, c, top_n, cand=None):
    users, kw = section_args(c)
    cand = cand or (c["cand_ptr"], c["cand_item"])
    return (t.rank_topn(users, top_n, candidates=cand, **kw), t.rank_positions(users, c["pos_ptr"], c["pos_item"], candidates=cand, **kw))


def ban_both(t, c, top_n):
    """the old calls ranking the same sets: the complement of each as bans"""
    users, kw = section_args(c)
    return (t.rank_topn(users, top_n, *c["ban_topn"], **kw), t.rank_positions(users, c["pos_ptr"], c["pos_item"], *c["ban_pos"], **kw))


def assert_both_same(got, want):
    assert_same(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


_trained = {}


def trained(tmp, kind, k):
    """a model of width k after one training pass -- plain, user-group (feedback lists) or with both side tables (USER lines; a user-group
    trainer with feedback lists as well at k = 16 and 128) --, its sections, and the old calls' results on the complement bans, taken BEFORE
    any candidate call; computed once and shared (nothing below changes them)"""
    if (kind, k) not in _trained:
        fmt = 1 if kind == "feedback" or (kind == "lines" and k in (16, 128)) else 0
        pairs, tu, ti = (), None, None
        if kind == "lines":
            d = tmp / ("tables_%d" % k)
            d.mkdir()
            pairs, tu, ti = write_tables(d, "hand", NU, NI)
        t = lines_trainer(NU, NI, k, fmt, pairs)
        if fmt == 1:
            for b in training_input(k, fmt, NI):
                t.update_block(b)
        else:
            t.update_batch(training_input(k, fmt, NI))
        users, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(NS, NU, NI, seed=k)
        c = dict(kind=kind, k=k, fmt=fmt, t=t, N=TOPS[k], users=users, pos_ptr=pos_ptr, pos_item=pos_item, cand_ptr=cand_ptr, cand_item=cand_item,
                 ban_pos=complement(NI, cand_ptr, cand_item, pos_ptr, pos_item), ban_topn=complement(NI, cand_ptr, cand_item), pairs=pairs)
        if fmt == 1:
            c["fb"] = make_feedback(NS, NFB, seed=k + 7)
        if kind == "lines":
            c["lines"] = make_lines(NS, NU, k + 3)
        U, W, bias = t.view("W_user").copy(), t.view("W_item").copy(), t.view("i_bias").copy()
        Wfb = t.view("W_ufeedback").copy() if fmt == 1 else None
        if kind == "lines":
            c["rows"] = rule_line_rows(U, c["lines"], tu, Wfb, c.get("fb"))
        elif kind == "feedback":
            c["rows"] = rule_user_rows(U, Wfb, users, *c["fb"])
        else:
            c["rows"] = U[users]
        c["W"], c["bias"] = rule_item_side(W, bias, ti)
        c["old"] = ban_both(t, c, c["N"])
        users_, kw = section_args(c)
        c["old_eval"] = t.rank_eval(users_, pos_ptr, pos_item, *c["ban_pos"], at=(1, 10), **kw)
        _trained[(kind, k)] = c
    return _trained[(kind, k)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_candidates_equal_complement_bans_and_the_rule(tmp, kind, k):
    """40 sections over 1 200 items: lists of 0, 1, 63, 64, 65, 129, 257 and all 1 200 ids and random ones, with duplicate ids, positives
    listed and not listed, a section without positives, user 7 in three sections.  Positions, `tied`, `ranked`, ids, counts, `nan` and the
    scores' bits equal the old calls' under complement bans AND the numpy rule; either form of the score kernel gives the same bits; the
    counters count; the old calls answer afterwards what they answered before"""
    c = trained(tmp, kind, k)
    t, N = c["t"], c["N"]
    before = [t.counter(w) for w in COUNTERS]
    got = cand_both(t, c, N)
    assert_both_same(got, c["old"])
    # 38: the sections with positives; 39: all; 40 / 41: rows with a feedback sum / built from a line, in either call; 42: 38 + 39 of these calls
    both = 2 * NS - 1
    assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [NS - 1, NS, both if c["fmt"] == 1 else 0, both if kind == "lines" else 0, both]
    want = (rule_cand_topn(c["rows"], c["W"], c["bias"], N, c["cand_ptr"], c["cand_item"]),
            rule_cand_positions(c["rows"], c["W"], c["bias"], c["pos_ptr"], c["pos_item"], c["cand_ptr"], c["cand_item"]))
    assert_both_same(got, want)
    assert not got[0][3].any() and not got[1][3].any() and (got[0][2] < N).any() and got[0][2][7] == min(N, NI)
    for form in (1, 2):
        t.set_knob("rank_cand_form", form)
        again = cand_both(t, c, N)
        t.set_knob("rank_cand_form", 0)
        assert_both_same(again, got)
    users, kw = section_args(c)
    position, tied, ranked, nan = got[1]
    m = t.rank_eval(users, c["pos_ptr"], c["pos_item"], at=(1, 10), candidates=(c["cand_ptr"], c["cand_item"]), **kw)
    assert m == sa.rank_metrics(c["pos_ptr"], position, ranked=ranked, nan=nan, at=(1, 10)) == c["old_eval"] and m["ninst"] == NS - 1
    # the old calls on the same trainer, after the candidate calls
    mid = [t.counter(w) for w in COUNTERS]
    assert_both_same(ban_both(t, c, N), c["old"])
    assert t.rank_eval(users, c["pos_ptr"], c["pos_item"], *c["ban_pos"], at=(1, 10), **kw) == c["old_eval"]
    assert t.counter(42) == mid[4] and t.counter(38) - mid[0] == 2 * (NS - 1) and t.counter(39) - mid[1] == NS


@pytest.mark.parametrize("top_n", [1, 10, 256])
def test_every_top_n_on_one_model(tmp, top_n):
    c = trained(tmp, "users", 128)
    users, kw = section_args(c)
    got = c["t"].rank_topn(users, top_n, candidates=(c["cand_ptr"], c["cand_item"]), **kw)
    assert_same(got, c["t"].rank_topn(users, top_n, *c["ban_topn"], **kw))
    assert_same(got, rule_cand_topn(c["rows"], c["W"], c["bias"], top_n, c["cand_ptr"], c["cand_item"]))
    distinct = np.array([len(np.unique(c["cand_item"][a:b])) for a, b in zip(c["cand_ptr"][:-1], c["cand_ptr"][1:])])
    np.testing.assert_array_equal(got[2], np.minimum(top_n, distinct))


@pytest.mark.parametrize("k", [64, 320])
def test_a_nan_row_flags_only_the_sections_that_rank_it(tmp, k):
    """item `bad` gets a NaN row: it is inside the sets of some sections (as a candidate or as a positive) and outside the others'"""
    c = trained(tmp, "users", k)
    t = c["t"]
    sets = [np.union1d(c["cand_item"][c["cand_ptr"][s]:c["cand_ptr"][s + 1]], c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]]) for s in range(NS)]
    lists = [np.unique(c["cand_item"][c["cand_ptr"][s]:c["cand_ptr"][s + 1]]) for s in range(NS)]
    bad = int(lists[3][1])
    in_set = np.array([bad in x for x in sets]).astype(np.int32)
    in_list = np.array([bad in x for x in lists]).astype(np.int32)
    assert 2 <= in_list.sum() < NS - 10 and in_set[7] and in_set[3]
    W = t.view("W_item").copy()
    keep = W[bad].copy()
    W[bad, k // 2] = np.nan
    t.set_view("W_item", W)
    (items, scores, count, nan), (position, tied, ranked, pnan) = cand_both(t, c, c["N"])
    W[bad] = keep
    t.set_view("W_item", W)
    in_set[NOPOS] = 0                                   # nothing of a section without positives is scored
    np.testing.assert_array_equal(nan, in_list)
    np.testing.assert_array_equal(pnan, in_set)
    got = cand_both(t, c, c["N"])                       # the model is what it was
    assert_both_same(got, c["old"])
    for s in range(NS):
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        if in_list[s]:
            assert count[s] == 0 and (items[s] == -1).all() and (scores[s] == 0).all()
        else:
            np.testing.assert_array_equal(items[s], got[0][0][s])
        if in_set[s]:
            assert (position[a:b] == -1).all() and (tied[a:b] == -1).all()
        else:
            np.testing.assert_array_equal(position[a:b], got[1][0][a:b])
    np.testing.assert_array_equal(ranked, got[1][2])


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_rounding_is_pinned(k):
    """the rounding input of tests/test_rank_cand.py (rank_rounding's clustered rows: the scores of a section lie a few ulp apart): the
    results equal the rule in the pinned order, in either form of the score kernel, and differ from the rule under every wrong summation order"""
    c = rounding_input(k)
    t = lines_trainer(c["nu"], c["ni"], k, 0)
    for name, key in (("W_item", "W"), ("W_user", "U"), ("i_bias", "bias")):
        t.set_view(name, c[key])
    cc = dict(c, kind="users")
    want = rounding_results(k, "pinned")
    for form in (0, 1, 2):
        t.set_knob("rank_cand_form", form)
        got = cand_both(t, cc, c["N"])
        assert_both_same(got, want)
    for wrong in DOT_DECOYS:
        other = rounding_results(k, wrong)
        assert (got[0][0] != other[0][0]).any(axis=1).sum() >= 1, wrong
        assert (got[1][0] != other[1][0]).sum() >= 1, wrong


@pytest.mark.parametrize("kind, k", [("users", 64), ("lines", 128)])
def test_results_do_not_depend_on_the_pieces(tmp, kind, k):
    """rank_eval_budget lowered until either call takes several pieces, with the catalogue-sized list larger than the budget: a piece of its
    own.  Candidate entries count towards the knob in both kinds of call"""
    c = trained(tmp, kind, k)
    t = c["t"]
    want = cand_both(t, c, c["N"])
    total = len(np.concatenate([np.unique(c["cand_item"][a:b]) for a, b in zip(c["cand_ptr"][:-1], c["cand_ptr"][1:])]))
    for budget in (1000, 300, 1):
        assert NI > budget and total >= 3 * budget
        before = [t.counter(w) for w in COUNTERS]
        launches = t.counter(1)
        t.set_knob("rank_eval_budget", budget)
        got = cand_both(t, c, c["N"])
        t.set_knob("rank_eval_budget", 1 << 22)
        assert_both_same(got, want)
        assert [t.counter(w) - b for w, b in zip(COUNTERS, before)][:2] == [NS - 1, NS] and t.counter(42) - before[4] == 2 * NS - 1
        assert t.counter(1) - launches >= 2 * 2 * 3          # at least 3 pieces per call, two launches each


def ranker_lists(c, path, top_k, ban_ptr, ban_item):
    """every section through the CPU ranker on the saved model with top_k = N: a USER line, a BAN line of the complement, a PROCESS line"""
    r = oracle.OracleRanker("reference" if oracle.have_reference() else "port", 0, 0)
    r.set_param("top_k", str(top_k))
    r.load_model(path)
    r.init_ranker(NI)
    r.process_rows(sa.CSRData.from_rows([(0.0, [], [], [(i, 1.0)]) for i in range(NI)]))
    out = {}
    for s in range(NS):
        b = ban_item[ban_ptr[s]:ban_ptr[s + 1]]
        if NI - len(b) < top_k:
            continue                                       # the reference asserts: k can not exceed candidate size
        rows = [(2.0, [], [(int(c["users"][s]), 1.0)], [])]
        if len(b):
            rows.append((-1.0, [], [(int(x), 1.0) for x in b], []))
        rows.append((4.0, [], [], []))
        out[s] = np.asarray(r.process_rows(sa.CSRData.from_rows(rows)))
    return out


def test_results_equal_the_cpu_ranker(tmp, tmp_path):
    """the saved model through the CPU ranker, item set = the catalogue, bans = the complement: positions equal on every untied positive,
    lists on every section without a tie among its top_n + 1 best; at least 90 % of each are compared (tests/test_rank_cand.py asserts that
    the input allows it)"""
    c = trained(tmp, "users", ROUTE_K)
    t, N = c["t"], ROUTE_N
    assert N == c["N"]
    (items, _, count, _), (position, tied, _, _) = cand_both(t, c, N)
    path = str(tmp_path / "m.model")
    t.save_model(path)
    want = port_positions(path, NI, c["users"], c["pos_ptr"], c["pos_item"], *c["ban_pos"])
    assert len(want) == len(position) and (tied == 0).mean() >= 0.9
    np.testing.assert_array_equal(position[tied == 0], want[tied == 0])
    more = t.rank_topn(c["users"], N + 1, candidates=(c["cand_ptr"], c["cand_item"]))
    compared, full = 0, 0
    for s, w in ranker_lists(c, path, N, *c["ban_topn"]).items():
        assert len(w) == N == count[s]
        full += 1
        if (np.diff(more[1][s, :more[2][s]]) < 0).all():
            compared += 1
            np.testing.assert_array_equal(w, items[s], err_msg=str(s))
    assert full >= NS - 4 and compared >= 0.9 * full


def test_lists_are_refused_before_any_launch(tmp):
    c = trained(tmp, "users", 64)
    t = c["t"]
    before = [t.counter(w) for w in COUNTERS]
    launches = t.counter(1)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_topn([1, 2], 5, candidates=([0, 1, 3], [3, NI, 4]))
    with pytest.raises(sa.SvdfError, match="rank_eval: cand_ptr must not decrease"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], candidates=([0, 3, 2], [3, 19, 4]))
    with pytest.raises(sa.SvdfError, match="rank_topn: bans and candidates exclude each other"):
        t.rank_topn([1, 2], 5, [0, 0, 1], [3], candidates=([0, 1, 3], [3, 5, 4]))
    # no section, and a positions call without any positive: nothing is launched
    assert t.rank_topn([], 5, candidates=([0], []))[0].shape == (0, 5)
    position, tied, ranked, nan = t.rank_positions([1, 2], [0, 0, 0], [], candidates=([0, 3, 5], [1, 2, 2, 8, 29]))
    assert len(position) == 0 and ranked.tolist() == [2, 2] and nan.tolist() == [0, 0]
    assert [t.counter(w) for w in COUNTERS] == before and t.counter(1) == launches

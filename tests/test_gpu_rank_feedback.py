"""Live-model ranking for user-group (SVD++) trainers on the GPU (svdf_rank_*_fb, svdf_k_rankrows.hip).  The checker is the numpy
statement of the rule in tests/test_rank_feedback.py -- ids, positions and the scores' bits must be equal -- and, for the agreement of the
routes, the pinned port's ranker (the compiled reference where it has been built) fed every section as one block."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from test_gpu_rank_eval import new_trainer
from test_gpu_rank_topn import assert_same
from test_rank_feedback import (EMPTY, LONG, NFB, NI, NS, NU, ROUNDING_KS, ROW_DECOYS, fb_conf, make_feedback, rounding_input, rounding_results,
                                rule_lists, rule_pos, rule_user_rows, section_lists, training_blocks)

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = [7, 16, 64, 128, 200, 320]            # the tail, every class of lane group the row kernel dispatches, and the wide rows
TOPS = {7: 10, 16: 64, 64: 10, 128: 100, 200: 256, 320: 1}
VIEWS = ("u_bias", "W_user", "i_bias", "W_item", "ufeedback_bias", "W_ufeedback")


def fb_trainer(nu, ni, k, nfb=NFB, seed=3, ext=0):
    """a user-group trainer; k = 16 trains rank_blocks under the rank loss of PAIR_CONF"""
    pairs = k == 16
    t = sa.Trainer(1, 3 if pairs else 0, ext)
    t.seed(seed)
    for kk, v in fb_conf(nu, ni, k, base=cases.PAIR_CONF if pairs else cases.BASICMF_CONF, num_ufeedback=nfb):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    return t


def model_of(t):
    return dict(U=t.view("W_user").copy(), W=t.view("W_item").copy(), bias=t.view("i_bias").copy(), Wfb=t.view("W_ufeedback").copy())


def both(t, c, top_n, fb="fb"):
    """the two calls on the lists of c: (rank_topn's tuple, rank_positions' tuple)"""
    feedback = c[fb] if isinstance(fb, str) else fb
    return (t.rank_topn(c["users"], top_n, c["ban_ptr"], c["ban_item"], feedback=feedback),
            t.rank_positions(c["users"], c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"], feedback=feedback))


def assert_both_same(got, want):
    assert_same(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


_trained = {}


def trained(k, ni=NI):
    """the model of width k after one pass of user blocks, its sections and both results, computed once and shared (nothing below changes them)"""
    if (k, ni) not in _trained:
        t = fb_trainer(NU, ni, k, ext=1 if k == 128 else 0)
        for b in training_blocks(k):
            t.update_block(b)
        c = section_lists(k, ni)
        before = [t.counter(w) for w in (38, 39, 40)]
        got = both(t, c, TOPS[k])                    # straight after the staged pass
        c.update(t=t, got=got, counted=[t.counter(w) - b for w, b in zip((38, 39, 40), before)], N=TOPS[k], **model_of(t))
        _trained[(k, ni)] = c
    return _trained[(k, ni)]


def rule_both(c, order="pinned", fb=None):
    rows = rule_user_rows(c["U"], c["Wfb"], c["users"], *(fb or c["fb"]), order=order)
    return rule_lists(rows, c["W"], c["bias"], c["N"], c["ban_ptr"], c["ban_item"]), rule_pos(rows, c["W"], c["bias"], c["pos_ptr"], c["pos_item"],
                                                                                                c["ban_ptr"], c["ban_item"])


@pytest.mark.parametrize("k, ni", [pytest.param(k, NI, id=str(k)) for k in KS] + [pytest.param(64, 1200, id="64-1200items")])
def test_lists_and_positions_equal_the_rule(k, ni):
    """lists of 0 .. 40 entries, one of 300, an empty one, repeated ids; 150 sections; with 1 200 items the sweeps split them over two item
    ranges.  Scores bit for bit; the feedback rows have been trained"""
    c = trained(k, ni)
    lists, (position, tied) = rule_both(c)
    assert_same(c["got"][0], lists)
    np.testing.assert_array_equal(c["got"][1][0], position)
    np.testing.assert_array_equal(c["got"][1][1], tied)
    assert not c["got"][0][3].any() and not c["got"][1][3].any()
    n = np.diff(c["fb"][0])
    assert n[LONG] == 300 and n[EMPTY] == 0
    assert c["counted"] == [NS - 1, NS, 2 * NS - 1]          # 38: the sections with positives; 39: all; 40: both calls built their rows from lists
    fresh = fb_trainer(NU, ni, k)
    assert not np.array_equal(fresh.view("W_ufeedback"), c["Wfb"])


def port_results(c, path, top_k):
    """every section as one block (its feedback list; USER, POS, BAN and PROCESS lines) through the CPU ranker on the saved model"""
    r = oracle.OracleRanker("reference" if oracle.have_reference() else "port", 1, 0)
    r.set_param("top_k", str(top_k))
    r.load_model(path)
    ni = len(c["W"])
    r.init_ranker(ni)
    r.process_rows(sa.CSRData.from_rows([(0.0, [], [], [(i, 1.0)]) for i in range(ni)]))
    fb_ptr, fb_index, fb_value = c["fb"]
    out = {}
    for s in range(NS):
        p = c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]]
        b = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]]
        nban = len(np.unique(b))
        if (top_k == 0 and len(p) == 0) or (top_k and ni - nban < top_k):
            continue                                   # the reference asserts: no positive record / k can not exceed candidate size
        rows = [(2.0, [], [(int(c["users"][s]), 1.0)], [])]
        if len(p):
            rows.append((1.0, [], [(int(x), 1.0) for x in p], []))
        if len(b):
            _, first = np.unique(b, return_index=True)
            rows.append((-1.0, [], [(int(x), 1.0) for x in np.asarray(b)[np.sort(first)]], []))
        rows.append((4.0, [], [], []))
        blk = sa.PlusBlock(fb_index[fb_ptr[s]:fb_ptr[s + 1]], fb_value[fb_ptr[s]:fb_ptr[s + 1]], sa.CSRData.from_rows(rows), 0)
        out[s] = np.asarray(r.process_block(blk))
    return out


@pytest.mark.parametrize("k", [64, 128])
def test_results_equal_the_cpu_rankers(k, tmp_path):
    """the saved model through the pinned port's ranker (the compiled reference where it exists): positions equal on every untied positive,
    lists on every section without a tie among its top_n + 1 best; at least 90 % of each are compared (tests/test_rank_feedback.py asserts
    that the input allows it)"""
    c = trained(k)
    t, N = c["t"], c["N"]
    (items, _, count, _), (position, tied, _, _) = c["got"]
    path = str(tmp_path / "m.model")
    t.save_model(path)
    want = port_results(c, path, 0)
    npos = 0
    for s, w in want.items():
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        assert len(w) == b - a
        keep = tied[a:b] == 0
        npos += int(keep.sum())
        np.testing.assert_array_equal(position[a:b][keep], w[keep], err_msg=str(s))
    assert npos >= 0.9 * len(position)
    more = t.rank_topn(c["users"], N + 1, c["ban_ptr"], c["ban_item"], feedback=c["fb"])
    compared = 0
    for s, w in port_results(c, path, N).items():
        assert len(w) == N == count[s]
        if (np.diff(more[1][s, :more[2][s]]) < 0).all():
            compared += 1
            np.testing.assert_array_equal(w, items[s], err_msg=str(s))
    assert compared >= 0.9 * NS


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_rounding_is_pinned(k):
    """the rounding input of tests/test_rank_feedback.py (scores a few ulp apart, feedback rows of mixed magnitude): the results equal the rule
    in the pinned order and differ from the rule under every decoy of the user sum -- fused multiply-add, the list backwards, the user row first"""
    c = rounding_input(k)
    t = fb_trainer(c["nu"], c["ni"], k, nfb=c["nfb"])
    for name, key in (("W_item", "W"), ("W_user", "U"), ("i_bias", "bias"), ("W_ufeedback", "Wfb")):
        t.set_view(name, c[key])
    got = both(t, c, c["N"])
    want = rounding_results(c, "pinned")
    assert_same(got[0], want[0])
    np.testing.assert_array_equal(got[1][0], want[1][0])
    np.testing.assert_array_equal(got[1][1], want[1][1])
    for decoy in ROW_DECOYS:
        other = rounding_results(c, decoy)
        assert (got[0][0] != other[0][0]).any(axis=1).sum() >= 1, decoy
        assert (got[1][0] != other[1][0]).sum() >= 1, decoy


@pytest.mark.parametrize("k", [64, 320])
def test_empty_lists_are_the_old_call_on_a_plain_trainer(k):
    """every list empty: the row is 0 + W_user[u] * 1, and the results are, bit for bit, the OLD calls' on a format_type = 0 trainer that holds
    the same W_user, W_item, i_bias"""
    c = trained(k)
    plain = new_trainer(NU, NI, k, seed=5)
    for name in ("W_user", "W_item", "i_bias"):
        plain.set_view(name, c["t"].view(name))
    none = (np.zeros(NS + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, F32))
    before = c["t"].counter(40)
    got = both(c["t"], c, c["N"], fb=none)
    assert c["t"].counter(40) - before == 2 * NS - 1
    assert_both_same(got, both(plain, c, c["N"], fb=None))
    assert plain.counter(40) == 0
    assert not np.array_equal(got[0][0], c["got"][0][0])       # (and the lists DO matter)
    # a _fb call without lists on the plain trainer is the old call
    assert_both_same(both(plain, c, c["N"], fb=(None, None, None)), got)


def test_results_do_not_depend_on_the_pieces():
    """rank_eval_budget and rank_topn_budget lowered until either call takes at least three pieces (the feedback entries count towards the
    first in both calls): the results are those of the one-piece call, and counter 40 rose by the sections ranked"""
    c = trained(64)
    t = c["t"]
    nfb = int(c["fb"][0][-1])
    assert nfb > 3 * 700
    for knobs in ({"rank_eval_budget": 700}, {"rank_topn_budget": 5 * 512}, {"rank_eval_budget": 300, "rank_topn_budget": 40 * 512}):
        before = [t.counter(w) for w in (38, 39, 40)]
        for name, v in knobs.items():
            t.set_knob(name, v)
        got = both(t, c, c["N"])
        t.set_knob("rank_eval_budget", 1 << 22)
        t.set_knob("rank_topn_budget", 1 << 25)
        assert_both_same(got, c["got"])
        rose = [t.counter(w) - b for w, b in zip((38, 39, 40), before)]
        assert rose == [NS - 1, NS, 2 * NS - 1], (knobs, rose)    # top-N: 40 rose by S; evaluation: by the S - 1 sections that have positives


def test_straight_after_an_unsynchronised_pass():
    """trained(k) ranked straight after its staged pass: the result is that of a second handle given the model read back after synchronize"""
    c = trained(128)
    t = c["t"]
    t.synchronize()
    ref = fb_trainer(NU, NI, 128, seed=77)
    assert not np.array_equal(ref.view("W_item"), t.view("W_item"))
    for name in VIEWS:
        ref.set_view(name, t.view(name))
    assert_both_same(both(ref, c, c["N"]), c["got"])


def test_a_nan_value_flags_the_sections_whose_list_holds_it():
    c = trained(64)
    fb_ptr, fb_index, fb_value = c["fb"]
    n, npos = np.diff(fb_ptr), np.diff(c["pos_ptr"])
    bad = [s for s in (3, 64, LONG, NS - 1) if n[s] > 0 and npos[s] > 0]
    assert len(bad) >= 3 and LONG in bad
    value = fb_value.copy()
    for s in bad:
        value[fb_ptr[s] + n[s] // 2] = np.nan
    (items, scores, count, nan), (position, tied, ranked, pnan) = both(c["t"], c, c["N"], fb=(fb_ptr, fb_index, value))
    flags = np.zeros(NS, np.int32)
    flags[bad] = 1
    np.testing.assert_array_equal(nan, flags)
    np.testing.assert_array_equal(pnan, flags)
    for s in range(NS):
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        if flags[s]:
            assert count[s] == 0 and (items[s] == -1).all() and (scores[s] == 0).all() and (position[a:b] == -1).all()
        else:                                             # every other section is what it was
            np.testing.assert_array_equal(items[s], c["got"][0][0][s])
            np.testing.assert_array_equal(position[a:b], c["got"][1][0][a:b])
    np.testing.assert_array_equal(ranked, c["got"][1][2])


def test_lists_are_refused_before_any_launch():
    t = fb_trainer(20, 30, 8, nfb=30)
    with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
        t.rank_topn([1, 2], 5, feedback=([0, 2, 3], [3, 30, 4], [0.5, -1.0, 2.0]))
    with pytest.raises(sa.SvdfError, match="rank_eval: fb_ptr must not decrease"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], feedback=([0, 3, 2], [3, 29, 4], [0.5, -1.0, 2.0]))
    with pytest.raises(sa.SvdfError, match="rank_topn: fb_ptr is NULL on a user-group trainer"):
        t.rank_topn([1, 2], 5, feedback=(None, None, None))
    with pytest.raises(sa.SvdfError, match="rank_topn: user-group trainers"):
        t.rank_topn([1, 2], 5)
    assert t.counter(39) == t.counter(40) == 0
    items, scores, count, nan = t.rank_topn([1, 1], 40, [0, 3, 5], [7, 7, 8, 5, 5], feedback=([0, 0, 3], [3, 3, 29], [0.5, -1.0, 2.0]))
    assert count.tolist() == [28, 29] and t.counter(39) == t.counter(40) == 2 and not nan.any()
    assert not np.array_equal(scores[0, :5], scores[1, :5])      # one user, two lists, two rankings

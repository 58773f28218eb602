"""Live-model ranking for sections with USER lines and trainers with side tables on the GPU (svdf_rank_*_lines, svdf_k_rankrows.hip; DESIGN.md
6z).  The checker is the numpy statement of the rule in tests/test_rank_lines.py -- ids, counts, positions, `tied` and the scores' bits must
be equal -- and, for the agreement of the routes, the CPU ranker (the compiled reference where it has been built) on the saved model with
the same tables, fed every section as USER / POS / BAN / PROCESS lines."""
import numpy as np
import pytest

import svdfeature_amd as sa
from oracle import oracle
from test_gpu_rank_feedback import TOPS
from test_gpu_rank_topn import assert_same
from test_rank_lines import (EMPTY, ITEM_WRONG, LONG, NI, NS, NU, ROUNDING_KS, ROUTE_CASES, ROW_WRONG, lines_conf, rounding_input, rounding_results,
                             rule_both, section_lists, training_input, unit_lines, write_rounding_tables, write_tables)

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = (38, 39, 40, 41)
# (width, format_type, tables, items): every table set -- both tables (written by hand, generated), feature_user only, feature_item only,
# neither -- on both kinds of trainer at every width (the tail, each class of lane group, a wide row); 1 200 items: the sweeps split them
# over two item ranges
KS = (7, 16, 64, 128, 200, 320)
RULE_CASES = ([(k, fmt, which, NI) for k in KS for fmt in (0, 1) for which in ("hand", "generated", "user", "item", "none")] +
              [(64, 0, "hand", 1200), (200, 1, "generated", 1200)])


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("rank_lines")


def lines_trainer(nu, ni, k, fmt, tables=(), seed=3):
    t = sa.Trainer(fmt, 0, 1 if fmt == 1 and k == 128 else 0)
    t.seed(seed)
    for kk, v in lines_conf(nu, ni, k, fmt, tables):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    return t


def both(t, c, top_n, lines=None, fb="fb"):
    """the two _lines calls on the lists of c: (rank_topn's tuple, rank_positions' tuple)"""
    kw = dict(lines=lines or c["lines"], feedback=c.get(fb) if isinstance(fb, str) else fb)
    return (t.rank_topn(None, top_n, c["ban_ptr"], c["ban_item"], **kw),
            t.rank_positions(None, c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"], **kw))


def assert_both_same(got, want):
    assert_same(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


_trained = {}


def trained(tmp, k, fmt, which, ni=NI):
    """the model of width k after one training pass with the tables set, its sections and both results, computed once and shared (nothing
    below changes them)"""
    key = (k, fmt, which, ni)
    if key not in _trained:
        d = tmp / ("%d_%d_%s_%d" % key)
        d.mkdir()
        pairs, tu, ti = write_tables(d, which, NU, ni)
        t = lines_trainer(NU, ni, k, fmt, pairs)
        fresh = t.view("W_user").copy()
        if fmt == 1:
            for b in training_input(k, fmt, ni):
                t.update_block(b)
        else:
            t.update_batch(training_input(k, fmt, ni))
        c = section_lists(k, NU, ni, fb=fmt == 1)
        before = [t.counter(w) for w in COUNTERS]
        got = both(t, c, TOPS[k])                    # straight after the training pass
        c.update(t=t, got=got, counted=[t.counter(w) - b for w, b in zip(COUNTERS, before)], N=TOPS[k], fmt=fmt, pairs=pairs, table_u=tu, table_i=ti,
                 fresh=fresh, U=t.view("W_user").copy(), W=t.view("W_item").copy(), bias=t.view("i_bias").copy())
        if fmt == 1:
            c["Wfb"] = t.view("W_ufeedback").copy()
        _trained[key] = c
    return _trained[key]


@pytest.mark.parametrize("k, fmt, which, ni", [pytest.param(*p, id="%d-fmt%d-%s%s" % (p[:3] + ("-1200items" if p[3] != NI else "",))) for p in RULE_CASES])
def test_lists_and_positions_equal_the_rule(tmp, k, fmt, which, ni):
    """150 sections: lines u:1, an empty one, three ids with a negative value and 1 +- 5e-7, a repeated id, one of 300 ids (with feedback lists
    on the user-group trainer); ids, counts, positions, `tied` and the scores' bits; the metrics of the positions are svdf_rank_eval_lines'"""
    c = trained(tmp, k, fmt, which, ni)
    lists, (position, tied) = rule_both(c, c["N"])
    assert_same(c["got"][0], lists)
    np.testing.assert_array_equal(c["got"][1][0], position)
    np.testing.assert_array_equal(c["got"][1][1], tied)
    assert not c["got"][0][3].any() and not c["got"][1][3].any()
    n = np.diff(c["lines"][0])
    assert n[LONG] == 300 and n[EMPTY] == 0
    # 38: the sections with positives; 39: all; 40: rows that hold a feedback sum; 41: both calls built their rows from lines
    assert c["counted"] == [NS - 1, NS, 2 * NS - 1 if fmt == 1 else 0, 2 * NS - 1]
    assert (c["fresh"] != c["U"]).any()
    position, tied, ranked, nan = c["got"][1]
    m = c["t"].rank_eval(None, c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"], at=(1, 10), lines=c["lines"], feedback=c.get("fb"))
    assert m == sa.rank_metrics(c["pos_ptr"], position, ranked=ranked, nan=nan, at=(1, 10)) and m["ninst"] == NS - 1


@pytest.mark.parametrize("k", [64, 320])
def test_unit_lines_without_tables_are_the_old_calls(tmp, k):
    """lines u:1 on trainers without tables: bit for bit the old calls (format_type = 0) and the _fb calls (a user-group trainer)"""
    for fmt in (0, 1):
        c = trained(tmp, k, fmt, "none")
        t = c["t"]
        users = np.random.default_rng(k).integers(0, NU, NS).astype(np.uint32)
        before = [t.counter(w) for w in COUNTERS]
        got = both(t, c, c["N"], lines=unit_lines(users))
        assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [NS - 1, NS, 2 * NS - 1 if fmt == 1 else 0, 2 * NS - 1]
        fb = c.get("fb")
        old = (t.rank_topn(users, c["N"], c["ban_ptr"], c["ban_item"], feedback=fb),
               t.rank_positions(users, c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"], feedback=fb))
        assert t.counter(41) - before[3] == 2 * NS - 1            # the old calls do not count under 41
        assert_both_same(got, old)
        assert not np.array_equal(got[0][0], c["got"][0][0])      # (and the lines DO matter)


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_rounding_is_pinned(tmp, k):
    """the rounding input of tests/test_rank_lines.py (scores a few ulp apart, both tables): the results equal the rule in the pinned order and
    differ from the rule under every wrong order of the user row and of the item side"""
    c = rounding_input(k)
    d = tmp / ("rounding_%d" % k)
    d.mkdir()
    t = lines_trainer(c["nu"], c["ni"], k, 0, write_rounding_tables(c, d))
    for name, key in (("W_item", "W"), ("W_user", "U"), ("i_bias", "bias")):
        t.set_view(name, c[key])
    got = both(t, c, c["N"])
    want = rounding_results(k, "pinned")
    assert_same(got[0], want[0])
    np.testing.assert_array_equal(got[1][0], want[1][0])
    np.testing.assert_array_equal(got[1][1], want[1][1])
    for wrong in ROW_WRONG + ITEM_WRONG:
        other = rounding_results(k, wrong)
        assert (got[0][0] != other[0][0]).any(axis=1).sum() >= 1, wrong
        assert (got[1][0] != other[1][0]).sum() >= 1, wrong


def ranker_results(c, path, top_k):
    """every section (its USER line; POS, BAN and PROCESS lines; its feedback list on a user-group model) through the CPU ranker on the saved
    model with the same tables"""
    r = oracle.OracleRanker("reference" if oracle.have_reference() else "port", c["fmt"], 0)
    for kk, v in c["pairs"] + [("top_k", str(top_k))]:
        r.set_param(kk, v)
    r.load_model(path)
    ni = len(c["W"])
    r.init_ranker(ni)
    r.process_rows(sa.CSRData.from_rows([(0.0, [], [], [(i, 1.0)]) for i in range(ni)]))
    ul_ptr, ul_index, ul_value = c["lines"]
    out = {}
    for s in range(NS):
        p = c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]]
        b = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]]
        if (top_k == 0 and len(p) == 0) or (top_k and ni - len(np.unique(b)) < top_k):
            continue                                   # the reference asserts: no positive record / k can not exceed candidate size
        rows = [(2.0, [], [(int(i), float(v)) for i, v in zip(ul_index[ul_ptr[s]:ul_ptr[s + 1]], ul_value[ul_ptr[s]:ul_ptr[s + 1]])], [])]
        if len(p):
            rows.append((1.0, [], [(int(x), 1.0) for x in p], []))
        if len(b):
            _, first = np.unique(b, return_index=True)
            rows.append((-1.0, [], [(int(x), 1.0) for x in np.asarray(b)[np.sort(first)]], []))
        rows.append((4.0, [], [], []))
        data = sa.CSRData.from_rows(rows)
        if c["fmt"] == 1:
            fb_ptr, fb_index, fb_value = c["fb"]
            out[s] = np.asarray(r.process_block(sa.PlusBlock(fb_index[fb_ptr[s]:fb_ptr[s + 1]], fb_value[fb_ptr[s]:fb_ptr[s + 1]], data, 0)))
        else:
            out[s] = np.asarray(r.process_rows(data))
    return out


@pytest.mark.parametrize("k, fmt, which, top_n", ROUTE_CASES)
def test_results_equal_the_cpu_rankers(tmp, k, fmt, which, top_n, tmp_path):
    """positions equal on every untied positive, lists on every section without a tie among its top_n + 1 best; at least 90 % of each are
    compared (tests/test_rank_lines.py asserts that the input allows it)"""
    c = trained(tmp, k, fmt, which)
    t, N = c["t"], c["N"]
    assert N == top_n
    (items, _, count, _), (position, tied, _, _) = c["got"]
    path = str(tmp_path / "m.model")
    t.save_model(path)
    npos = 0
    for s, w in ranker_results(c, path, 0).items():
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        assert len(w) == b - a
        keep = tied[a:b] == 0
        npos += int(keep.sum())
        np.testing.assert_array_equal(position[a:b][keep], w[keep], err_msg=str(s))
    assert npos >= 0.9 * len(position)
    more = t.rank_topn(None, N + 1, c["ban_ptr"], c["ban_item"], lines=c["lines"], feedback=c.get("fb"))
    compared = 0
    for s, w in ranker_results(c, path, N).items():
        assert len(w) == N == count[s]
        if (np.diff(more[1][s, :more[2][s]]) < 0).all():
            compared += 1
            np.testing.assert_array_equal(w, items[s], err_msg=str(s))
    assert compared >= 0.9 * NS


def test_counters_and_the_old_calls_on_a_side_table_trainer(tmp):
    """the old six calls still refuse a trainer with side tables, in their words, and move no counter; the _lines calls count under 38 / 39
    and 41 (and 40 on a user-group trainer)"""
    for fmt in (0, 1):
        c = trained(tmp, 64, fmt, "hand")
        t, users, fb = c["t"], np.arange(NS, dtype=np.uint32) % NU, c.get("fb")
        before = [t.counter(w) for w in COUNTERS]
        for call in (lambda: t.rank_topn(users, 5, feedback=fb), lambda: t.rank_positions(users, c["pos_ptr"], c["pos_item"], feedback=fb),
                     lambda: t.rank_eval(users, c["pos_ptr"], c["pos_item"], feedback=fb)):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): feature_user / feature_item side tables change the score"):
                call()
        assert [t.counter(w) for w in COUNTERS] == before
        items, scores, count, nan = t.rank_topn(None, 5, lines=([0, 1, 1, 3], [1, 2, 2], [1.0, 0.5, -1.0]), feedback=([0, 0, 2, 2], [3, 4], [0.5, 0.5]) if fmt else None)
        assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [0, 3, 3 if fmt else 0, 3] and (count == 5).all() and not nan.any()
        assert t.rank_topn(None, 5, lines=([0], [], []), feedback=([0], [], []) if fmt else None)[0].shape == (0, 5)      # no section: nothing launched
        assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [0, 3, 3 if fmt else 0, 3]


def test_results_do_not_depend_on_the_pieces(tmp):
    """rank_eval_budget and rank_topn_budget lowered until either call takes several pieces (line entries count towards the first in both
    calls): the results are those of the one-piece call; the prepared item side is built once per call"""
    c = trained(tmp, 64, 1, "hand")
    t = c["t"]
    assert int(c["lines"][0][-1]) > 500
    for knobs in ({"rank_eval_budget": 200}, {"rank_topn_budget": 5 * 512}, {"rank_eval_budget": 150, "rank_topn_budget": 40 * 512}):
        before = [t.counter(w) for w in COUNTERS]
        for name, v in knobs.items():
            t.set_knob(name, v)
        got = both(t, c, c["N"])
        t.set_knob("rank_eval_budget", 1 << 22)
        t.set_knob("rank_topn_budget", 1 << 25)
        assert_both_same(got, c["got"])
        assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [NS - 1, NS, 2 * NS - 1, 2 * NS - 1], knobs


def test_a_nan_value_flags_the_sections_whose_line_holds_it(tmp):
    c = trained(tmp, 64, 0, "hand")
    ul_ptr, ul_index, ul_value = c["lines"]
    n, npos = np.diff(ul_ptr), np.diff(c["pos_ptr"])
    bad = [s for s in (3, 64, LONG, NS - 1) if n[s] > 0 and npos[s] > 0]
    assert len(bad) >= 3 and LONG in bad
    value = ul_value.copy()
    for s in bad:
        value[ul_ptr[s] + n[s] // 2] = np.nan
    (items, scores, count, nan), (position, tied, ranked, pnan) = both(c["t"], c, c["N"], lines=(ul_ptr, ul_index, value))
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


def test_lines_are_refused_before_any_launch(tmp):
    c = trained(tmp, 64, 0, "hand")
    t = c["t"]
    before = [t.counter(w) for w in COUNTERS]
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_topn(None, 5, lines=([0, 1, 3], [3, NU, 4], [1.0, -1.0, 2.0]))
    with pytest.raises(sa.SvdfError, match="rank_eval: ul_ptr must not decrease"):
        t.rank_positions(None, [0, 2, 3], [5, 6, 7], lines=([0, 3, 2], [3, 19, 4], [1.0, -1.0, 2.0]))
    with pytest.raises(sa.SvdfError, match="rank_topn: feedback lists need a user-group trainer"):
        t.rank_topn(None, 5, lines=([0, 1, 3], [3, 19, 4], [1.0, -1.0, 2.0]), feedback=([0, 1, 2], [3, 4], [0.5, 0.5]))
    assert [t.counter(w) for w in COUNTERS] == before

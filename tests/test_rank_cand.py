"""Live-model ranking over per-section candidate lists, the parts that need no GPU: the numpy statement of the rule for a
ranked set that tests/test_gpu_rank_cand.py compares the GPU against; the host list functions (svdf_rankcand_lists.h) through the stand-alone
tool tools/check_rankcand_lists.cpp; the conditions on the inputs that test shares (found and asserted here, on the CPU); and every refusal of
the svdf_rank_*_cand calls that is decided before the device, on a host-only handle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from rank_rounding import DOT_DECOYS, cluster, score_fp32
from test_rank_eval import host_trainer
from test_rank_feedback import ptr_of
from test_rank_lines import lines_conf, training_input

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, NI, NS = 200, 1200, 40
LENGTHS = (0, 1, 63, 64, 65, 129, 257, NI)      # the candidate lists of the sections 0 .. 7: around one, two and four tiles of 64, the catalogue
NOPOS = 9                                        # the section without positives
SAME_USER = (0, NS // 4, NS // 2)                # user 7 in three sections with different lists


# ---- the rule
def ranked_set(cand, pos=()):
    """the distinct ids of a section's candidate list together with its positives, ascending"""
    return np.unique(np.concatenate([np.asarray(cand, np.int64), np.asarray(pos, np.int64)]))


def rule_cand_positions(rows, W, bias, pos_ptr, pos_item, cand_ptr, cand_item, order="pinned"):
    """(position, tied, ranked, nan) of Trainer.rank_positions(..., candidates=...) by the documented rule: only the ranked set of a section
    is scored (rank_rounding.score_fp32: one float32 operation at a time, `order` the pinned summation order or a decoy's); position =
    strictly higher + tied with a smaller id, +0 == -0, NaN equals nothing; a NaN among the RANKED scores flags the section (-1, -1)"""
    position, tied = [], []
    ranked, nan = np.zeros(len(rows), np.int32), np.zeros(len(rows), np.int32)
    for s in range(len(rows)):
        pos = np.asarray(pos_item[pos_ptr[s]:pos_ptr[s + 1]], np.int64)
        ids = ranked_set(cand_item[cand_ptr[s]:cand_ptr[s + 1]], pos)
        ranked[s] = len(ids)
        if len(pos) == 0:
            continue
        sc = score_fp32(rows[s], W[ids], bias[ids], order)
        if np.isnan(sc).any():
            nan[s] = 1
            position += [-1] * len(pos)
            tied += [-1] * len(pos)
            continue
        for p in pos:
            t = sc[np.searchsorted(ids, p)]
            eq = (sc == t) & (ids != p)
            position.append(int((sc > t).sum() + (eq & (ids < p)).sum()))
            tied.append(int(eq.sum()))
    return np.array(position, np.int32), np.array(tied, np.int32), ranked, nan


def rule_cand_topn(rows, W, bias, top_n, cand_ptr, cand_item, order="pinned"):
    """(items, scores, count, nan) of Trainer.rank_topn(..., candidates=...) by the rule: the distinct ids of the list alone, higher score
    first, equal scores by ascending id with -0 folded onto +0; a NaN among them flags the section, whose list is then empty"""
    S = len(rows)
    items, scores = np.full((S, top_n), -1, np.int32), np.zeros((S, top_n), F32)
    count, nan = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s in range(S):
        ids = ranked_set(cand_item[cand_ptr[s]:cand_ptr[s + 1]])
        v = score_fp32(rows[s], W[ids], bias[ids], order)
        if np.isnan(v).any():
            nan[s] = 1
            continue
        v = np.where(v == 0, F32(0.0), v)
        o = np.lexsort((ids, -v))[:top_n]
        count[s] = len(o)
        items[s, :len(o)], scores[s, :len(o)] = ids[o], v[o]
    return items, scores, count, nan


def complement(ni, cand_ptr, cand_item, pos_ptr=None, pos_item=None):
    """the ban lists under which the old calls rank the same sets: per section every id that is in neither list"""
    ban = []
    for s in range(len(cand_ptr) - 1):
        keep = ranked_set(cand_item[cand_ptr[s]:cand_ptr[s + 1]], pos_item[pos_ptr[s]:pos_ptr[s + 1]] if pos_ptr is not None else ())
        ban.append(np.setdiff1d(np.arange(ni), keep).astype(np.uint32))
    return ptr_of(ban), np.concatenate(ban)


# ---- the sections of the GPU tests
def make_candidates(S, nu, ni, seed, lengths=LENGTHS, nopos=NOPOS):
    """S sections: (users, pos_ptr, pos_item, cand_ptr, cand_item).  The lists of the first sections have the lengths `lengths`, the others
    2 .. 300 ids; every third list repeats some of its ids; 1 - 4 positives per section (section `nopos` none), each listed among the
    candidates or not by a coin; user 7 in three sections with different lists"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    users[list(SAME_USER)] = 7
    cand, pos = [], []
    for s in range(S):
        n = lengths[s] if s < len(lengths) else int(rng.integers(2, 301))
        c = rng.permutation(ni)[:n]
        npos = 0 if s == nopos else int(rng.integers(1, 5))
        p = np.array([int(c[rng.integers(0, n)]) if n and rng.integers(0, 2) else int(rng.integers(0, ni)) for _ in range(npos)], np.int64)
        p = np.unique(p)
        if s % 3 == 0 and n > 2:
            c = np.concatenate([c, c[:int(rng.integers(1, 4))]])       # duplicate ids count once
            c = c[rng.permutation(len(c))]
        cand.append(c.astype(np.uint32))
        pos.append(p.astype(np.uint32))
    return users, ptr_of(pos), np.concatenate(pos), ptr_of(cand), np.concatenate(cand)


def test_the_rule_on_a_hand_made_case():
    """six items whose scores are their biases (zero factor rows): item 5 scores best but is in no list; a tie (1, 2); a +-0 pair (3, 4); a
    positive that is listed twice and one that is not listed; an empty list; a NaN outside one section's set and inside another's"""
    W, rows = np.zeros((7, 4), F32), np.ones((4, 4), F32)
    bias = np.array([1.0, 2.0, 2.0, -0.0, 0.0, 3.0, np.nan], F32)
    cand_ptr, cand_item = [0, 5, 5, 8, 10], [2, 0, 2, 3, 4, 1, 2, 5, 6, 0]
    pos_ptr, pos_item = [0, 2, 3, 4, 5], [2, 1, 0, 1, 0]
    position, tied, ranked, nan = rule_cand_positions(rows, W, bias, pos_ptr, pos_item, cand_ptr, cand_item)
    # section 0 ranks {0 1 2 3 4}: 2 ties with 1 and has the larger id; section 1 {0}; section 2 {1 2 5}; section 3 {0 6} holds the NaN
    assert position.tolist() == [1, 0, 0, 1, -1] and tied.tolist() == [1, 1, 0, 1, -1]
    assert ranked.tolist() == [5, 1, 3, 2] and nan.tolist() == [0, 0, 0, 1]
    items, scores, count, nan = rule_cand_topn(rows, W, bias, 4, cand_ptr, cand_item)
    assert items.tolist() == [[2, 0, 3, 4], [-1] * 4, [5, 1, 2, -1], [-1] * 4] and count.tolist() == [4, 0, 3, 0] and nan.tolist() == [0, 0, 0, 1]
    assert np.signbit(scores[0]).tolist() == [False] * 4                      # -0 is listed as +0
    # the same sets as bans of the complement
    ban_ptr, ban_item = complement(7, cand_ptr, cand_item, pos_ptr, pos_item)
    assert [ban_item[a:b].tolist() for a, b in zip(ban_ptr[:-1], ban_ptr[1:])] == [[5, 6], [1, 2, 3, 4, 5, 6], [0, 3, 4, 6], [1, 2, 3, 4, 5]]


def test_the_sections_cover_what_the_issue_names():
    users, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(NS, NU, NI, seed=64)
    n = np.diff(cand_ptr)
    assert n[:2].tolist() == [0, 1] and len(np.unique(cand_item[cand_ptr[7]:cand_ptr[8]])) == NI      # an empty list, the whole catalogue
    distinct = [len(np.unique(cand_item[a:b])) for a, b in zip(cand_ptr[:-1], cand_ptr[1:])]
    assert distinct[:8] == list(LENGTHS) and any(d < m for d, m in zip(distinct, n))          # duplicate ids
    listed = [np.isin(pos_item[pos_ptr[s]:pos_ptr[s + 1]], cand_item[cand_ptr[s]:cand_ptr[s + 1]]) for s in range(NS)]
    assert any(x.any() for x in listed) and any((~x).any() for x in listed)                    # positives listed and not listed
    assert pos_ptr[NOPOS] == pos_ptr[NOPOS + 1] and pos_ptr[1] > pos_ptr[0]                    # positives with an empty list
    assert (users[list(SAME_USER)] == 7).all() and min(distinct) < 10 < 256 < max(distinct)    # lists shorter and longer than top_n


# ---- the host list functions, through the stand-alone tool
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler to build tools/check_rankcand_lists.cpp with"
    exe = str(tmp_path_factory.mktemp("rankcand") / "check_rankcand_lists")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "svdfeature_amd", "csrc"),
                           os.path.join(ROOT, "tools", "check_rankcand_lists.cpp"), "-o", exe])
    return exe


def dump(tool, ni, cand, pos=None):
    text = "%d %d %d\n" % (len(cand), ni, pos is not None)
    for s in range(len(cand)):
        for part in [cand[s]] + ([pos[s]] if pos is not None else []):
            text += " ".join(str(int(x)) for x in [len(part)] + list(part)) + "\n"
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout
    if out.startswith("refused"):
        return out.strip()
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}


def test_the_tool_passes_its_own_checks(tool):
    assert subprocess.run([tool], capture_output=True, text=True).stdout.strip() == "ok"


@pytest.mark.parametrize("positions", [True, False])
def test_host_lists_dedupe_union_indices_and_tiles(tool, positions):
    """the ranked sets are the sorted distinct ids (with the positives in a positions call, where only sections with positives are kept),
    every positive's index points at its id, and the tiles hold at most 64 consecutive pairs of one section"""
    _, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(NS, NU, NI, seed=7)
    cand = [cand_item[a:b] for a, b in zip(cand_ptr[:-1], cand_ptr[1:])]
    pos = [pos_item[a:b] for a, b in zip(pos_ptr[:-1], pos_ptr[1:])]
    got = dump(tool, NI, cand, pos if positions else None)
    sets = [ranked_set(c, p if positions else ()) for c, p in zip(cand, pos)]
    assert got["ranked"] == [len(x) for x in sets]
    kept = [x if (not positions or len(p)) else x[:0] for x, p in zip(sets, pos)]
    assert got["ids"] == np.concatenate(kept).tolist() and got["first"] == ptr_of(kept).tolist()
    if positions:
        assert [got["ids"][at] for at in got["pos_at"]] == pos_item.tolist()
        assert all(got["first"][s] <= at < got["first"][s + 1] for s in range(NS) for at in got["pos_at"][pos_ptr[s]:pos_ptr[s + 1]])
    else:
        assert got["pos_at"] == []
    q0, sec = got["tile_q0"], got["tile_sec"]
    assert q0[0] == 0 and q0[-1] == len(got["ids"]) and len(q0) == len(sec) + 1
    for t, s in enumerate(sec):
        assert 1 <= q0[t + 1] - q0[t] <= 64 and got["first"][s] <= q0[t] and q0[t + 1] <= got["first"][s + 1]
    assert sum(1 for s in range(NS) if len(kept[s])) == len(set(sec)) and len(sec) == sum((len(x) + 63) // 64 for x in kept)
    assert dump(tool, 10, [[1, 10]], [[2]]) == "refused sample item index exceed bound"
    assert dump(tool, 10, [[1, 2]], [[3, 3]]) == "refused rank_eval: a positive item is repeated inside a section"


# ---- the rounding input: clustered item rows (one base row +- 800 ulp per element), so that the scores of a section lie a few ulp apart
ROUNDING_KS = (64, 200, 320)               # the staged form with 64 and with 16 rows in a turn, the one-lane form of the wide rows
_rounding = {}


def rounding_input(k):
    if k not in _rounding:
        nu, ni, S, N = 40, 500, 40, 50
        rng = np.random.default_rng(700 + k)
        W = cluster(rng, ni, k, 800)
        U = rng.standard_normal((nu, k)).astype(F32)
        users, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(S, nu, ni, seed=k + 1, lengths=(0, 1, 63, 64, 65, 129, 257, ni))
        _rounding[k] = dict(nu=nu, ni=ni, S=S, N=N, k=k, U=U, W=W, bias=np.zeros(ni, F32), users=users, pos_ptr=pos_ptr, pos_item=pos_item,
                            cand_ptr=cand_ptr, cand_item=cand_item)
    return _rounding[k]


_rounding_results = {}


def rounding_results(k, order):
    if (k, order) not in _rounding_results:
        c = rounding_input(k)
        rows = c["U"][c["users"]]
        _rounding_results[(k, order)] = (rule_cand_topn(rows, c["W"], c["bias"], c["N"], c["cand_ptr"], c["cand_item"], order),
                                         rule_cand_positions(rows, c["W"], c["bias"], c["pos_ptr"], c["pos_item"], c["cand_ptr"], c["cand_item"], order))
    return _rounding_results[(k, order)]


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_the_rounding_input_sees_every_wrong_order(k):
    """under each of rank_rounding's summation decoys the rule gives another list for some section and another position for some positive"""
    lists, pos = rounding_results(k, "pinned")
    for wrong in DOT_DECOYS:
        other = rounding_results(k, wrong)
        assert (lists[0] != other[0][0]).any(axis=1).sum() >= 1, wrong
        assert (pos[0] != other[1][0]).sum() >= 1, wrong


# ---- the route-agreement input: a plain model trained by one pass through the pinned port
ROUTE_K, ROUTE_N = 64, 10
_route = {}


def route_input():
    if not _route:
        t = oracle.OracleTrainer("port", 0, 0)
        t.seed(3)
        for kk, v in lines_conf(NU, NI, ROUTE_K, 0):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        t.update_batch(training_input(ROUTE_K, 0, NI))
        users, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(NS, NU, NI, seed=ROUTE_K)
        _route.update(users=users, pos_ptr=pos_ptr, pos_item=pos_item, cand_ptr=cand_ptr, cand_item=cand_item, U=t.view("W_user").copy(),
                      W=t.view("W_item").copy(), bias=t.view("i_bias").copy(), N=ROUTE_N)
        t.close()
    return _route


def test_the_route_agreement_input_is_mostly_untied():
    """what the comparison with the CPU ranker relies on, from the rule alone: at least 90 % of the positives are untied and at least 90 % of
    the sections that list top_n candidates have no tie among their top_n + 1 best"""
    c = route_input()
    rows = c["U"][c["users"]]
    _, tied, _, nan = rule_cand_positions(rows, c["W"], c["bias"], c["pos_ptr"], c["pos_item"], c["cand_ptr"], c["cand_item"])
    assert not nan.any() and (tied == 0).mean() >= 0.9
    _, scores, count, _ = rule_cand_topn(rows, c["W"], c["bias"], c["N"] + 1, c["cand_ptr"], c["cand_item"])
    full = count >= c["N"]
    untied = np.array([(np.diff(scores[s, :count[s]]) < 0).all() for s in range(NS)])
    assert full.sum() >= NS - 4 and untied[full].mean() >= 0.9


# ---- refusals on host-only handles
POS = ([0, 2, 3], [5, 6, 7])
CAND = ([0, 3, 5], [1, 2, 2, 8, 29])
UL = ([0, 1, 3], [3, 19, 4], [1.0, -1.0, 2.0])
FB = ([0, 2, 3], [3, 29, 4], [0.5, -1.0, 2.0])
USERS = [1, 2]


def calls(t, users, cand, lines=None, fb=None, pos=POS):
    """the three methods with one candidates argument"""
    kw = dict(candidates=cand, lines=lines, feedback=fb)
    return [lambda: t.rank_positions(users, *pos, **kw), lambda: t.rank_eval(users, *pos, **kw), lambda: t.rank_topn(users, 5, **kw)]


def group_trainer(ext=0, extra=(), **kw):
    return host_trainer(fmt=1, ext=ext, extra=[("num_ufeedback", 30)] + list(extra), **kw)


def side_tables(tmp_path):
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n0\n2 4:0.25 4:0.5\n")
    return [[("feature_user", str(table))], [("feature_item", str(table))], [("feature_user", str(table)), ("feature_item", str(table))]]


def test_a_legal_call_on_a_host_only_handle_needs_a_gpu(tmp_path):
    """every way of naming the sections, with an empty list, duplicate ids, a list that covers the catalogue and no section at all"""
    legal = ([0, 0, 34], [4, 4] + list(range(30)) + [0, 29])
    t0, t1 = host_trainer(), group_trainer(1)
    for cand in (CAND, legal):
        for call in calls(t0, USERS, cand) + calls(t0, None, cand, lines=UL) + calls(t1, USERS, cand, fb=FB) + calls(t1, None, cand, lines=UL, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn) needs a GPU"):
                call()
    for call in calls(t0, [], ([0], []), pos=([0], [])):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn) needs a GPU"):
            call()
    for extra in side_tables(tmp_path):
        for call in calls(host_trainer(extra=extra), None, CAND, lines=UL) + calls(group_trainer(extra=extra), None, CAND, lines=UL, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn) needs a GPU"):
                call()
        # with users the side tables are refused in the twins' words
        for call in calls(host_trainer(extra=extra), USERS, CAND) + calls(group_trainer(extra=extra), USERS, CAND, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): feature_user / feature_item side tables change the score"):
                call()
    assert t0.counter(42) == t1.counter(42) == t0.counter(38) == t0.counter(39) == 0


def test_candidate_list_refusals_come_before_the_device():
    t = host_trainer()
    for j, who in enumerate(("rank_eval", "rank_eval", "rank_topn")):       # rank_positions, rank_eval, rank_topn
        call = lambda cand, j=j, **kw: calls(t, USERS, cand, **kw)[j]()
        with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
            call(([0, 3, 5], [1, 2, 2, 8, 30]))
        with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
            call(([0, 3, 5], [1, 4000000000, 2, 8, 29]))
        with pytest.raises(sa.SvdfError, match=who + ": cand_ptr must not decrease"):
            call(([0, 3, 2], [1, 2, 2, 8, 29]))
        with pytest.raises(sa.SvdfError, match=who + ": cand_ptr must start at >= 0"):
            call(([-1, 3, 5], [1, 2, 2, 8, 29]))
        with pytest.raises(sa.SvdfError, match=who + ": cand_ptr is missing"):
            call((None, None))
        with pytest.raises(sa.SvdfError, match=who + ": cand_item is missing"):
            call(([0, 3, 5], None))
        with pytest.raises(sa.SvdfError, match=who + ": cand_ptr must have one entry more than there are sections"):
            call(([0, 3], [1, 2, 2]))
        with pytest.raises(sa.SvdfError, match=who + ": cand_item is shorter than cand_ptr says"):
            call(([0, 3, 5], [1, 2, 2]))
        with pytest.raises(sa.SvdfError, match=who + ": bans and candidates exclude each other"):
            [t.rank_positions, t.rank_eval, lambda u, *a, **kw: t.rank_topn(u, 5, **kw)][j](USERS, *(POS if j < 2 else ()), ban_ptr=[0, 0, 1], ban_item=[3],
                                                                                             candidates=CAND)
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            calls(t, [1, 20], CAND)[j]()
        with pytest.raises(sa.SvdfError, match=who + ": with lines= the sections bring USER lines: users must be None"):
            calls(t, USERS, CAND, lines=UL)[j]()
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            calls(t, None, CAND, lines=([0, 1, 3], [3, 20, 4], [1.0, -1.0, 2.0]))[j]()
        with pytest.raises(sa.SvdfError, match=who + ": feedback lists need a user-group trainer"):
            calls(t, USERS, CAND, fb=FB)[j]()
    # the positives keep the twins' refusals; a positive may be listed among the candidates
    with pytest.raises(sa.SvdfError, match="rank_eval: a positive item is repeated inside a section"):
        t.rank_positions(USERS, [0, 2, 3], [5, 5, 7], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions(USERS, [0, 2, 3], [5, 30, 7], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="rank_eval: pos_ptr must not decrease"):
        t.rank_positions(USERS, [0, 2, 1], [5, 6, 7], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="rank_eval: pos_ptr must have one entry more than users"):
        t.rank_positions(USERS, [0, 2], [5, 6], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="rank_eval needs a GPU"):
        t.rank_positions(USERS, [0, 2, 3], [1, 2, 8], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_topn(USERS, 257, candidates=CAND)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_topn(USERS, 0, candidates=CAND)
    # the feedback triple keeps section 6y's refusals
    g = group_trainer()
    for call in calls(g, USERS, CAND) + calls(g, None, CAND, lines=UL):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): fb_ptr is NULL on a user-group trainer.*explicitly as an empty list"):
            call()
    for call in calls(g, USERS, CAND, fb=([0, 2, 3], [3, 30, 4], [0.5, -1.0, 2.0])):
        with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
            call()
    assert t.counter(38) == t.counter(39) == t.counter(42) == g.counter(42) == 0


def test_null_pointers_through_the_c_entry_points():
    t = host_trainer()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    users, cptr, citem = np.array(USERS, np.uint32), np.array(CAND[0], np.int64), np.array(CAND[1], np.uint32)
    ul = [np.array(UL[0], np.int64), np.array(UL[1], np.uint32), np.array(UL[2], F32)]
    pos_ptr, pos_item, out = np.array(POS[0], np.int64), np.array(POS[1], np.uint32), [np.zeros(3, np.int32) for _ in range(4)]
    items, count, nan = np.zeros(10, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    m, at = sa.RankMetrics(), np.array([5], np.int32)
    none3 = [None, None, None]
    for who, msg in (([None] + none3, "give the sections either as users or as USER lines"),
                     ([p(users)] + [p(a) for a in ul], "give the sections either as users or as USER lines")):
        assert t.lib.svdf_rank_topn_cand(t.h, 2, *who, *none3, p(cptr), p(citem), 5, items, None, count, nan) == -1
        assert "rank_topn: " + msg in t.lib.svdf_last_error().decode()
        assert t.lib.svdf_rank_eval_positions_cand(t.h, 2, *who, *none3, pos_ptr, pos_item, p(cptr), p(citem), *out) == -1
        assert "rank_eval: " + msg in t.lib.svdf_last_error().decode()
        assert t.lib.svdf_rank_eval_cand(t.h, 2, *who, *none3, pos_ptr, pos_item, p(cptr), p(citem), 1, at, C.byref(m)) == -1
        assert "rank_eval: " + msg in t.lib.svdf_last_error().decode()
    for cand, msg in (([None, p(citem)], "cand_ptr is missing"), ([p(cptr), None], "cand_item is missing")):
        assert t.lib.svdf_rank_topn_cand(t.h, 2, p(users), *none3, *none3, *cand, 5, items, None, count, nan) == -1
        assert "rank_topn: " + msg in t.lib.svdf_last_error().decode()
        assert t.lib.svdf_rank_eval_positions_cand(t.h, 2, None, *[p(a) for a in ul], *none3, pos_ptr, pos_item, *cand, *out) == -1
        assert "rank_eval: " + msg in t.lib.svdf_last_error().decode()
    assert t.lib.svdf_rank_topn_cand(t.h, 2, p(users), *none3, *none3, p(cptr), p(citem), 5, items, None, count, nan) == -1
    assert "rank_topn needs a GPU" in t.lib.svdf_last_error().decode()


def test_configuration_refusals_are_the_twins(tmp_path):
    for ext in (2, 15):
        for call in calls(sa.Trainer(1, 0, ext, device=-2), USERS, CAND, fb=FB) + calls(sa.Trainer(1, 0, ext, device=-2), None, CAND, lines=UL, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): user-group trainers .*extend_type != 0 are not covered"):
                call()
    for call in calls(host_trainer(extra=[("amd:gpus", 2)]), USERS, CAND):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): amd:gpus > 1 is not covered"):
            call()
    for call in calls(host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]), USERS, CAND):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): common_latent_space != 0"):
            call()
    with pytest.raises(sa.SvdfError, match="rank_topn: call init_model / load_model and init_trainer first"):
        sa.Trainer(0, 0, 0, device=-2).rank_topn(USERS, 5, candidates=CAND)


class Recorder:
    """the library with the names of the entry points a call reached"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        if name.startswith("svdf_rank_"):
            self.names.append(name)
        return getattr(self._lib, name)


def test_without_candidates_the_old_entry_points_are_reached():
    t, g = host_trainer(), group_trainer()
    for h in (t, g):
        h.lib = Recorder(h.lib)
    for call, want in ((lambda: t.rank_positions(USERS, *POS, candidates=None), "svdf_rank_eval_positions"),
                       (lambda: t.rank_eval(USERS, *POS), "svdf_rank_eval"), (lambda: t.rank_topn(USERS, 5, candidates=None), "svdf_rank_topn"),
                       (lambda: g.rank_positions(USERS, *POS, feedback=FB, candidates=None), "svdf_rank_eval_positions_fb"),
                       (lambda: g.rank_topn(USERS, 5, feedback=FB), "svdf_rank_topn_fb"),
                       (lambda: t.rank_positions(None, *POS, lines=UL, candidates=None), "svdf_rank_eval_positions_lines"),
                       (lambda: t.rank_eval(None, *POS, lines=UL), "svdf_rank_eval_lines"), (lambda: t.rank_topn(None, 5, lines=UL), "svdf_rank_topn_lines"),
                       (lambda: t.rank_positions(USERS, *POS, candidates=CAND), "svdf_rank_eval_positions_cand"),
                       (lambda: t.rank_eval(None, *POS, lines=UL, candidates=CAND), "svdf_rank_eval_cand"),
                       (lambda: g.rank_topn(USERS, 5, feedback=FB, candidates=CAND), "svdf_rank_topn_cand")):
        del t.lib.names[:], g.lib.names[:]
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call()
        assert t.lib.names + g.lib.names == [want]

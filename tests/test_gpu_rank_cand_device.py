"""The _cand calls with their sets built on the device (knob rank_cand_build = 1; svdf_k_rankcandsets.hip) against the same
calls on the same handle with the host build (knob 0: today's path, which tests/test_gpu_rank_cand.py holds against complement bans and the
numpy rule) and np.unique for the sets.  Every output array byte for byte, and the counters 58 .. 60 by the form rule stated here."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from test_gpu_rank_lines import lines_trainer
from test_gpu_rank_topn import assert_same
from test_rank_cand import NI, NS, NU, make_candidates
from test_rank_feedback import NFB, make_feedback, ptr_of
from test_rank_lines import make_lines

pytestmark = pytest.mark.gpu
K, USERS_N, TOP = 8, 40, 10
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193)   # raw lengths: candidates + positives


def set_form(n, ni, force):
    """the form that builds a section of n raw ids: 1 sort (n <= 8192), 2 bitmap (num_item <= 524 288), 0 neither; force 0: the bitmap from
    the host's threshold 8 n >= ceil(num_item / 64) on and for every n > 8192; an empty section is the sort form's"""
    sort, bitmap = n <= 8192, n > 0 and (ni + 31) // 32 <= 16384
    first = force == 2 or (force == 0 and (n > 8192 or 8 * n >= (ni + 63) // 64))
    return 2 if bitmap and (first or not sort) else (1 if sort else 0)


def sections(ni, longest):
    """per raw length n <= longest a section of n candidates without positives and one of n - 1 candidates and one positive (listed or not by
    turns); one id 300 times; 200 entries with exactly 64 distinct ids; the ids 0 and ni - 1; user 3 in two sections with different lists;
    an empty first and last section without positives; positives inside the list, outside it, and both"""
    rng = np.random.default_rng(ni)
    cand, pos = [[]], [[]]
    for i, n in enumerate(x for x in LENGTHS if x <= longest):
        cand.append(rng.integers(0, ni, n))
        pos.append([])
        if n:
            c = rng.integers(0, ni, n - 1)
            cand.append(c)
            pos.append([int(c[0])] if n > 1 and i % 2 else [int(rng.integers(0, ni))])
    pool = rng.permutation(ni)[:64]
    cand += [np.full(300, 17), np.concatenate([pool, rng.choice(pool, 136)]), np.array([ni - 1, 0, 5, ni - 1, 0]), np.array([0, ni - 1, 9]), []]
    pos += [[16], [int(pool[3]), int(np.setdiff1d(np.arange(200), pool)[0])], [0, ni - 1], [], []]
    users = rng.integers(0, USERS_N, len(cand)).astype(np.uint32)
    users[[-2, -3]] = 3
    cand, pos = [np.asarray(x, np.uint32) for x in cand], [np.asarray(x, np.uint32) for x in pos]
    return dict(users=users, kw={}, pos_ptr=ptr_of(pos), pos_item=np.concatenate(pos), cand_ptr=ptr_of(cand), cand_item=np.concatenate(cand))


_plain = {}


def plain(ni):
    if ni not in _plain:
        t = sa.Trainer(0, 0)
        t.seed(5)
        for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=USERS_N, num_item=ni, num_factor=K, ui_init_sigma=0.1):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        _plain[ni] = t
    return _plain[ni]


def both_builds(t, c, ni, force, budget=None):
    """top-N and positions with the host build, then with the device build; the sets' sizes against np.unique; the counters by the rule"""
    cand = (c["cand_ptr"], c["cand_item"])
    call = lambda: (t.rank_topn(c["users"], TOP, candidates=cand, **c["kw"]),
                    t.rank_positions(c["users"], c["pos_ptr"], c["pos_item"], candidates=cand, **c["kw"]))
    t.set_knob("rank_cand_build_form", force)
    before = [t.counter(w) for w in (58, 59, 60)]
    want = call()
    assert [t.counter(w) for w in (58, 59, 60)] == before                    # the default, 0: nothing of the device build runs
    t.set_knob("rank_cand_build", 1)
    if budget:
        t.set_knob("rank_eval_budget", budget)
    got = call()
    t.set_knob("rank_cand_build", 0)
    t.set_knob("rank_eval_budget", 1 << 22)
    assert_same(got[0], want[0])
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)
    lists = [c["cand_item"][a:b] for a, b in zip(c["cand_ptr"][:-1], c["cand_ptr"][1:])]
    poss = [c["pos_item"][a:b] for a, b in zip(c["pos_ptr"][:-1], c["pos_ptr"][1:])]
    assert got[1][2].tolist() == [len(np.unique(np.concatenate([x, p]))) for x, p in zip(lists, poss)]
    assert got[0][2].tolist() == [min(TOP, len(np.unique(x))) for x in lists] and not got[0][3].any() and not got[1][3].any()
    moved = [0, 0, 0]
    for forms in ([set_form(len(x), ni, force) for x in lists], [set_form(len(x) + len(p), ni, force) for x, p in zip(lists, poss)]):
        if 0 in forms:
            moved[2] += 1                                                    # the whole call takes the host build
        else:
            moved[0], moved[1] = moved[0] + forms.count(1), moved[1] + forms.count(2)
    assert [t.counter(w) - b for w, b in zip((58, 59, 60), before)] == moved
    return moved


@pytest.mark.parametrize("force", [0, 1, 2])
@pytest.mark.parametrize("longest", [8192, 8193])
@pytest.mark.parametrize("ni", [1025, 70000, 600000])
def test_device_built_sets_give_the_host_builds_bytes(ni, longest, force):
    """1 025 items: a ragged last bitmap word, the bitmap by rule from 3 ids on; 70 000: the sort form by rule up to 136 ids, the bitmap from
    137 on; 600 000: no bitmap, and 8 193 raw ids send the whole call to the host build"""
    c = sections(ni, longest)
    moved = both_builds(plain(ni), c, ni, force)
    if ni == 600000:
        assert moved == ([0, 0, 2] if longest == 8193 else [2 * len(c["users"]), 0, 0])
    else:
        assert moved[2] == 0 and moved[0] > 0 and (moved[1] > 0 or force == 1 and longest == 8192)


def test_three_pieces_give_the_same():
    ni = 70000
    c = sections(ni, 8192)
    t = plain(ni)
    launches = t.counter(1)
    both_builds(t, c, ni, 0, budget=9000)
    assert t.counter(1) - launches >= 2 * 3 * 4                              # either call: three pieces or more, four launches each


@pytest.mark.parametrize("force", [1, 2])
@pytest.mark.parametrize("kind", ["feedback", "lines", "feedback+lines"])
def test_the_rows_lists_travel_with_the_raw_lists(kind, force):
    """a user-group trainer with feedback= (and with both lists) and a plain one with lines=: the offsets of the rows' lists behind the raw
    ids in the upload -- of one piece, and of every piece where rank_eval_budget cuts the call into three or more"""
    t = lines_trainer(NU, NI, 16, 1 if "feedback" in kind else 0)
    users, pos_ptr, pos_item, cand_ptr, cand_item = make_candidates(NS, NU, NI, seed=21)
    kw = dict(feedback=make_feedback(NS, NFB, seed=5)) if "feedback" in kind else {}
    if "lines" in kind:
        kw["lines"] = make_lines(NS, NU, 9)
    c = dict(users=None if "lines" in kind else users, kw=kw, pos_ptr=pos_ptr, pos_item=pos_item, cand_ptr=cand_ptr, cand_item=cand_item)
    launches = t.counter(1)
    assert both_builds(t, c, NI, force)[2] == 0
    one_piece = t.counter(1) - launches
    # a quarter of the raw ids a piece, and no section alone holds more: four pieces or more.  The host build's calls run at the default
    # budget both times, so the launches that come on top are the device build's further pieces: sets, pack, rows and one or two of the
    # ranking, 4 or 5 a piece and call -- two pieces would add at most 2 * 5, three add at least 2 * 2 * 4
    raw = np.diff(cand_ptr) + np.diff(pos_ptr)
    budget = int(raw.sum()) // 4
    assert raw.max() <= budget
    launches = t.counter(1)
    assert both_builds(t, c, NI, force, budget=budget)[2] == 0
    assert t.counter(1) - launches - one_piece >= 2 * 2 * 4

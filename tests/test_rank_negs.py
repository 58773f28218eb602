"""Live-model ranking against negatives drawn on the device, the parts that need no GPU: the published rule in numpy
(tests/rank_negs_rule.py) against its pinned vectors and against the host export svdf_rank_negatives; the host list functions
(svdf_ranknegs_lists.h) through the stand-alone tool tools/check_ranknegs_lists.cpp; the sections tests/test_gpu_rank_negs.py shares; and
every refusal of the sampled calls, all decided before the device, on host-only handles."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import svdfeature_amd as sa
from rank_negs_rule import draws, rule_negatives, section_negatives, stream
from test_rank_cand import FB, POS, UL, USERS, Recorder, group_trainer, side_tables
from test_rank_eval import host_trainer
from test_rank_feedback import ptr_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, NI, NS = 200, 1200, 40
NOPOS = 9                          # the section without positives
SAME_USER = (0, NS // 4, NS // 2)  # user 7 in three sections with the same positives and bans
NEGS = (1, 63, 64, 65, 99, 500)    # around one round of 64 draws, and many rounds


def make_sections(S, nu, ni, seed, max_pos=3, nopos=NOPOS):
    """S sections: (users, pos_ptr, pos_item, ban_ptr, ban_item).  0 .. 190 banned ids per section, some of them repeated; 1 .. max_pos
    positives outside the bans (section `nopos` none); every fifth section bans what seed 12345 would draw first; user 7 in three sections
    that share their positives and bans"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    ban, pos = [], []
    for s in range(S):
        ids = rng.permutation(ni)
        p = ids[:0 if s == nopos else int(rng.integers(1, max_pos + 1))]
        b = ids[max_pos:max_pos + int(rng.integers(0, 191))]
        if s % 5 == 0 and len(p):
            first = draws(12345, s, 0, ni)
            if first not in p:
                b = np.append(b, first)
        if len(b) > 2:
            b = np.concatenate([b, b[:int(rng.integers(0, 4))]])                                # duplicate bans count once
            b = b[rng.permutation(len(b))]
        if s in SAME_USER[1:]:
            p, b = pos[SAME_USER[0]], ban[SAME_USER[0]]
        pos.append(p.astype(np.uint32))
        ban.append(b.astype(np.uint32))
    users[list(SAME_USER)] = 7
    return users, ptr_of(pos), np.concatenate(pos), ptr_of(ban), np.concatenate(ban)


def make_bans(pos_ptr, pos_item, ni, seed, first_seed=12345):
    """bans for GIVEN positives (the sections of tests/test_gpu_rank_cand.py's models): 0 .. 190 ids per section outside its positives, every
    third list with repeated ids, every fifth section banning what `first_seed` draws first; (ban_ptr, ban_item)"""
    rng = np.random.default_rng(seed)
    ban = []
    for s in range(len(pos_ptr) - 1):
        p = pos_item[pos_ptr[s]:pos_ptr[s + 1]]
        b = np.setdiff1d(rng.permutation(ni)[:int(rng.integers(0, 191))], p)
        first = draws(first_seed, s, 0, ni)
        if s % 5 == 0 and first not in p:
            b = np.append(b, first)
        if s % 3 == 0 and len(b) > 2:
            b = np.concatenate([b, b[:int(rng.integers(1, 4))]])
        ban.append(b[rng.permutation(len(b))].astype(np.uint32))
    return ptr_of(ban), np.concatenate(ban)


# ---- the rule
def test_the_pinned_vectors_of_the_rule():
    assert int(stream(12345, 0)) == 0x22118258a9d111a0 and int(stream(12345, 7)) == 0x6e7411b06820371c
    assert draws(12345, 0, np.arange(6), 1200).tolist() == [18, 601, 213, 846, 111, 362]
    assert draws(12345, 7, np.arange(8), 1200).tolist() == [1196, 25, 1196, 303, 504, 615, 588, 726]      # the third repeats the first
    neg, taken = section_negatives(12345, 7, 1200, 5, [25, 303])
    assert neg.tolist() == [1196, 504, 615, 588, 726] and taken == 8
    # the export: sections 0 and 7 with a positive each, section 7 banning 303 (twice) beside its positive 25
    pos_ptr, ban_ptr = [0, 1, 1, 1, 1, 1, 1, 1, 2], [0, 0, 0, 0, 0, 0, 0, 0, 2]
    got = sa.rank_negatives(1200, pos_ptr, [1199, 25], ban_ptr, [303, 303], 5, 12345)
    assert got.shape == (8, 5) and got.dtype == np.int32
    assert got[0].tolist() == [18, 601, 213, 846, 111] and got[7].tolist() == [1196, 504, 615, 588, 726] and (got[1:7] == -1).all()
    assert sa.rank_negatives(1200, pos_ptr, [1199, 25], None, None, 6, 12345)[0].tolist() == [18, 601, 213, 846, 111, 362]
    assert sa.rank_negatives(1200, pos_ptr, [1199, 25], None, None, 4, 12345)[7].tolist() == [1196, 303, 504, 615]


@pytest.mark.parametrize("num_neg", NEGS)
def test_the_export_equals_the_numpy_rule(num_neg):
    """300 sections over 1 200 items, bans of 0 .. 190 ids with duplicates, 0 .. 3 positives: the two statements of the rule agree; every id
    is in range, not excluded and distinct; a section without positives returns -1"""
    _, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(300, NU, NI, seed=num_neg)
    got = sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024)
    np.testing.assert_array_equal(got, rule_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024))
    for s in range(300):
        if pos_ptr[s] == pos_ptr[s + 1]:
            assert s == NOPOS and (got[s] == -1).all()
            continue
        ex = np.concatenate([pos_item[pos_ptr[s]:pos_ptr[s + 1]], ban_item[ban_ptr[s]:ban_ptr[s + 1]]])
        assert got[s].min() >= 0 and got[s].max() < NI and len(np.unique(got[s])) == num_neg and not np.isin(got[s], ex).any()
    # three sections with the same positives and bans (one user asked three times) get three lists
    a, b, c = (got[s] for s in SAME_USER)
    assert (pos_item[pos_ptr[SAME_USER[0]]:pos_ptr[SAME_USER[0] + 1]] == pos_item[pos_ptr[SAME_USER[2]]:pos_ptr[SAME_USER[2] + 1]]).all()
    if num_neg >= 63:
        assert (a != b).any() and (a != c).any() and (b != c).any()
    # the same seed gives the same lists, another seed others
    np.testing.assert_array_equal(got, sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024))
    other = sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2025)
    assert (other != got).any(axis=1).sum() >= 290
    # seeds are 64-bit: the high word matters, and the Python layer passes it
    assert (sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024 + (1 << 40)) != got).any()
    np.testing.assert_array_equal(sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024 + (1 << 40)),
                                  rule_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 2024 + (1 << 40)))


def test_the_sections_cover_what_the_issue_names():
    users, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(NS, NU, NI, seed=64)
    assert pos_ptr[NOPOS] == pos_ptr[NOPOS + 1] and (np.diff(pos_ptr) > 0).sum() == NS - 1 and (users[list(SAME_USER)] == 7).all()
    bans = [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    assert any(len(np.unique(b)) < len(b) for b in bans) and max(len(b) for b in bans) > 150                  # duplicated bans
    first = [int(draws(12345, s, 0, NI)) for s in range(NS)]
    assert sum(first[s] in bans[s] for s in range(NS)) >= 3                                                   # a ban that would be drawn first
    got = sa.rank_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, 99, 12345)
    assert all(first[s] not in got[s] for s in range(NS) if first[s] in bans[s])


def test_draws_are_about_uniform():
    """a condition, not a measurement: seed 99, 100 items, one negative, no bans, item 37 the positive of every one of 100 000 sections.  Each
    of the other 99 ids is expected 100 000 / 99 = 1 010 times; all counts lie within 15 % of that (the raw first draws, positive included,
    gave 918 .. 1 089 per id when the rule was written)"""
    S = 100000
    first = np.bincount(draws(99, np.arange(S), 0, 100), minlength=100)
    assert first.min() == 918 and first.max() == 1089
    neg = sa.rank_negatives(100, np.arange(S + 1), np.full(S, 37, np.uint32), None, None, 1, 99)
    count = np.bincount(neg.ravel(), minlength=100)
    expected = S / 99.0
    assert count[37] == 0 and count.sum() == S
    others = np.delete(count, 37)
    assert 0.85 * expected <= others.min() and others.max() <= 1.15 * expected, (others.min(), others.max())


# ---- the host list functions, through the stand-alone tool
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler to build tools/check_ranknegs_lists.cpp with"
    exe = str(tmp_path_factory.mktemp("ranknegs") / "check_ranknegs_lists")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-pthread", "-I", os.path.join(ROOT, "svdfeature_amd", "csrc"),
                           os.path.join(ROOT, "tools", "check_ranknegs_lists.cpp"), "-o", exe])
    return exe


def dump(tool, ni, num_neg, seed, ban, pos):
    text = "%d %d %d %d\n" % (len(pos), ni, num_neg, seed)
    for s in range(len(pos)):
        for part in (ban[s], pos[s]):
            text += " ".join(str(int(x)) for x in [len(part)] + list(part)) + "\n"
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout
    if out.startswith("refused"):
        return out.strip()
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()}


def test_the_tool_passes_its_own_checks(tool):
    assert subprocess.run([tool], capture_output=True, text=True).stdout.strip() == "ok"


@pytest.mark.parametrize("num_neg", [64, 99])
def test_host_lists_excluded_sets_offsets_and_tiles(tool, num_neg):
    """the excluded lists are the sorted distinct bans and positives of the sections with positives; a section's pairs are its positives
    and num_neg negatives, offsets from sizes alone; the tiles hold at most 64 consecutive pairs of one section; the negatives are the rule's"""
    _, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(NS, NU, NI, seed=7)
    ban = [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    pos = [pos_item[a:b] for a, b in zip(pos_ptr[:-1], pos_ptr[1:])]
    got = dump(tool, NI, num_neg, 5, ban, pos)
    ex = [np.unique(np.concatenate([b, p])) if len(p) else p[:0] for b, p in zip(ban, pos)]
    assert got["ex_ids"] == np.concatenate(ex).tolist() and got["ex_first"] == ptr_of(ex).tolist()
    size = [len(p) + num_neg if len(p) else 0 for p in pos]
    assert got["first"] == np.concatenate([[0], np.cumsum(size)]).tolist()
    assert got["ranked"] == [len(p) + num_neg for p in pos]
    assert got["neg"] == rule_negatives(NI, pos_ptr, pos_item, ban_ptr, ban_item, num_neg, 5).ravel().tolist()
    q0, sec = got["tile_q0"], got["tile_sec"]
    assert q0[0] == 0 and q0[-1] == sum(size) and len(q0) == len(sec) + 1 and len(sec) == sum((n + 63) // 64 for n in size)
    for t, s in enumerate(sec):
        assert 1 <= q0[t + 1] - q0[t] <= 64 and got["first"][s] <= q0[t] and q0[t + 1] <= got["first"][s + 1]
    assert dump(tool, 10, 2, 5, [[1, 10]], [[2]]) == "refused sample item index exceed bound"
    assert dump(tool, 10, 2, 5, [[1, 3]], [[3]]) == "refused each pos sample item can not occur in baned sample list"
    assert dump(tool, 10, 5, 5, [[1, 1]], [[3]]) == ("refused rank_eval: section 0 leaves 8 items to draw 5 negatives from 10; list its candidates "
                                                     "instead (svdf_rank_eval_positions_cand)")


# ---- refusals on host-only handles (30 items, 20 users)
BAN = ([0, 1, 3], [9, 10, 10])


def calls(t, users, sampled=(2, 5), lines=None, fb=None, pos=POS, ban=BAN, **kw):
    """the two methods (rank_positions also asking for the negatives) with one sampled argument"""
    kw = dict(kw, sampled=sampled, lines=lines, feedback=fb)
    ban = ban or (None, None)
    return [lambda: t.rank_positions(users, *pos, *ban, **kw), lambda: t.rank_positions(users, *pos, *ban, return_negatives=True, **kw),
            lambda: t.rank_eval(users, *pos, *ban, **kw)]


def test_a_legal_call_on_a_host_only_handle_needs_a_gpu(tmp_path):
    """every way of naming the sections, with and without bans, a section without positives, no section at all"""
    t0, t1 = host_trainer(), group_trainer(1)
    for ban in (BAN, None):
        for call in (calls(t0, USERS, ban=ban) + calls(t0, None, lines=UL, ban=ban) + calls(t1, USERS, fb=FB, ban=ban) +
                     calls(t1, None, lines=UL, fb=FB, ban=ban) + calls(t0, USERS, sampled=(13, 1 << 63), ban=ban)):
            with pytest.raises(sa.SvdfError, match="rank_eval needs a GPU"):
                call()
    for call in calls(t0, USERS, pos=([0, 0, 1], [5])) + calls(t0, [], pos=([0], []), ban=([0], [])):
        with pytest.raises(sa.SvdfError, match="rank_eval needs a GPU"):
            call()
    for extra in side_tables(tmp_path):
        for call in calls(host_trainer(extra=extra), None, lines=UL) + calls(group_trainer(extra=extra), None, lines=UL, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_eval needs a GPU"):
                call()
        # with users the side tables are refused in the twins' words
        for call in calls(host_trainer(extra=extra), USERS) + calls(group_trainer(extra=extra), USERS, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_eval: feature_user / feature_item side tables change the score"):
                call()
    assert t0.counter(43) == t1.counter(43) == t0.counter(38) == t0.counter(42) == 0


def test_sampled_refusals_come_before_the_device(tmp_path):
    t, g = host_trainer(), group_trainer()
    tabled = host_trainer(extra=side_tables(tmp_path)[2])
    handles = [(t, dict(users=USERS)), (g, dict(users=USERS, fb=FB)), (t, dict(users=None, lines=UL)), (g, dict(users=None, lines=UL, fb=FB)),
               (tabled, dict(users=None, lines=UL))]
    for h, who in handles:
        for j in range(3):
            call = lambda j=j, **kw: calls(h, **dict(who, **kw))[j]()
            for bad in (0, -1, 4097):
                with pytest.raises(sa.SvdfError, match="rank_eval: num_neg must be between 1 and 4096"):
                    call(sampled=(bad, 5))
            # 30 items: section 0 excludes {5, 6, 9}, 27 are left
            with pytest.raises(sa.SvdfError, match=r"rank_eval: section 0 leaves 27 items to draw 14 negatives from 30; list its candidates instead "
                                                   r"\(svdf_rank_eval_positions_cand\)"):
                call(sampled=(14, 5))
            with pytest.raises(sa.SvdfError, match="rank_eval: section 1 leaves 28 items to draw 15 negatives from 30"):
                call(sampled=(15, 5), pos=([0, 0, 2], [6, 7]), ban=None)       # a section without positives is not held to the rule
            with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
                call(ban=([0, 1, 3], [9, 30, 10]))
            with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
                call(pos=([0, 0, 1], [7]), ban=([0, 1, 1], [4000000000]))      # ... but its ids are validated
            with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
                call(pos=([0, 2, 3], [5, 30, 7]))
            with pytest.raises(sa.SvdfError, match="each pos sample item can not occur in baned sample list"):
                call(ban=([0, 1, 3], [6, 10, 10]))
            with pytest.raises(sa.SvdfError, match="rank_eval: a positive item is repeated inside a section"):
                call(pos=([0, 2, 3], [5, 5, 7]))
            with pytest.raises(sa.SvdfError, match="rank_eval: pos_ptr must not decrease"):
                call(pos=([0, 2, 1], [5, 6, 7]))
            with pytest.raises(sa.SvdfError, match="rank_eval: ban_ptr must not decrease"):
                call(ban=([0, 3, 1], [9, 10, 10]))
            with pytest.raises(sa.SvdfError, match="rank_eval: ban_ptr must start at >= 0"):
                call(ban=([-1, 1, 3], [9, 10, 10]))
            with pytest.raises(sa.SvdfError, match="rank_eval: ban_item is shorter than ban_ptr says"):
                call(ban=([0, 1, 3], None))
            with pytest.raises(sa.SvdfError, match="rank_eval: ban_item is shorter than ban_ptr says"):
                call(ban=([0, 1, 3], [9, 10]))
            with pytest.raises(sa.SvdfError, match="rank_eval: pos_item is shorter than pos_ptr says"):
                call(pos=([0, 2, 3], [5, 6]))
            with pytest.raises(sa.SvdfError, match="rank_eval: pos_ptr must have one entry more than users"):
                call(pos=([0, 2], [5, 6]))
            with pytest.raises(sa.SvdfError, match="rank_eval: ban_ptr must have one entry more than users"):
                call(ban=([0, 1], [9]))
            with pytest.raises(sa.SvdfError, match="rank_eval: candidates and sampled exclude each other"):
                call(candidates=([0, 3, 5], [1, 2, 2, 8, 29]), ban=None)
            with pytest.raises(sa.SvdfError, match="rank_eval: candidates and sampled exclude each other"):
                call(candidates=([0, 3, 5], [1, 2, 2, 8, 29]))
    for j in range(3):
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            calls(t, [1, 20])[j]()
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            calls(t, None, lines=([0, 1, 3], [3, 20, 4], [1.0, -1.0, 2.0]))[j]()
        with pytest.raises(sa.SvdfError, match="rank_eval: with lines= the sections bring USER lines: users must be None"):
            calls(t, USERS, lines=UL)[j]()
        with pytest.raises(sa.SvdfError, match="rank_eval: feedback lists need a user-group trainer"):
            calls(t, USERS, fb=FB)[j]()
        with pytest.raises(sa.SvdfError, match="rank_eval: fb_ptr is NULL on a user-group trainer.*explicitly as an empty list"):
            calls(g, USERS)[j]()
        with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
            calls(g, USERS, fb=([0, 2, 3], [3, 30, 4], [0.5, -1.0, 2.0]))[j]()
    with pytest.raises(sa.SvdfError, match="rank_eval: return_negatives needs sampled"):
        t.rank_positions(USERS, *POS, return_negatives=True)
    assert "sampled" not in sa.Trainer.rank_topn.__code__.co_varnames       # not offered on rank_topn
    assert t.counter(38) == t.counter(43) == g.counter(43) == tabled.counter(43) == 0


def test_the_host_export_refuses_in_the_same_words():
    with pytest.raises(sa.SvdfError, match="rank_eval: num_neg must be between 1 and 4096"):
        sa.rank_negatives(30, *POS, *BAN, 0, 5)
    with pytest.raises(sa.SvdfError, match="rank_eval: section 0 leaves 27 items to draw 14 negatives from 30; list its candidates instead"):
        sa.rank_negatives(30, *POS, *BAN, 14, 5)
    with pytest.raises(sa.SvdfError, match="rank_eval: section 0 leaves 1 items to draw 1 negatives from 100"):
        sa.rank_negatives(100, [0, 1], [0], [0, 98], np.arange(1, 99), 1, 5)                # avail >= 2 * num_neg
    assert sa.rank_negatives(100, [0, 1], [0], [0, 97], np.arange(1, 98), 1, 5).tolist() in ([[98]], [[99]])
    with pytest.raises(sa.SvdfError, match="rank_eval: section 0 leaves 18 items to draw 1 negatives from 1200"):
        sa.rank_negatives(1200, [0, 1], [0], [0, 1181], np.arange(1, 1182), 1, 5)           # avail * 64 >= num_item
    assert 1181 <= sa.rank_negatives(1200, [0, 1], [0], [0, 1180], np.arange(1, 1181), 1, 5)[0, 0] < 1200
    with pytest.raises(sa.SvdfError, match="rank_eval: ban_item is shorter than ban_ptr says"):
        sa.rank_negatives(30, *POS, [0, 1, 3], [9, 10], 2, 5)
    with pytest.raises(sa.SvdfError, match="rank_eval: pos_item is shorter than pos_ptr says"):
        sa.rank_negatives(30, [0, 2, 3], [5, 6], None, None, 2, 5)
    with pytest.raises(sa.SvdfError, match="each pos sample item can not occur in baned sample list"):
        sa.rank_negatives(30, *POS, [0, 1, 3], [6, 10, 10], 2, 5)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        sa.rank_negatives(30, *POS, [0, 1, 3], [9, 30, 10], 2, 5)
    with pytest.raises(sa.SvdfError, match="rank_eval: ban_ptr must have one entry more than users"):
        sa.rank_negatives(30, *POS, [0, 1], [9], 2, 5)
    with pytest.raises(sa.SvdfError, match="rank_eval: bad arguments"):
        sa.rank_negatives(0, *POS, *BAN, 2, 5)
    assert sa.rank_negatives(30, [0], [], None, None, 3, 5).shape == (0, 3)
    assert sa.rank_negatives(30, *POS, *BAN, 13, 5).shape == (2, 13)


def test_configuration_refusals_are_the_twins():
    for ext in (2, 15):
        for call in calls(sa.Trainer(1, 0, ext, device=-2), USERS, fb=FB) + calls(sa.Trainer(1, 0, ext, device=-2), None, lines=UL, fb=FB):
            with pytest.raises(sa.SvdfError, match="rank_eval: user-group trainers .*extend_type != 0 are not covered"):
                call()
    for call in calls(host_trainer(extra=[("amd:gpus", 2)]), USERS):
        with pytest.raises(sa.SvdfError, match="rank_eval: amd:gpus > 1 is not covered"):
            call()
    for call in calls(host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]), USERS):
        with pytest.raises(sa.SvdfError, match="rank_eval: common_latent_space != 0"):
            call()
    with pytest.raises(sa.SvdfError, match="rank_eval: call init_model / load_model and init_trainer first"):
        sa.Trainer(0, 0, 0, device=-2).rank_positions(USERS, *POS, sampled=(2, 5))


def test_without_sampled_the_old_entry_points_are_reached():
    t, g = host_trainer(), group_trainer()
    for h in (t, g):
        h.lib = Recorder(h.lib)
    cand = ([0, 3, 5], [1, 2, 2, 8, 29])
    for call, want in ((lambda: t.rank_positions(USERS, *POS, sampled=None), "svdf_rank_eval_positions"),
                       (lambda: t.rank_positions(USERS, *POS, *BAN, sampled=None, return_negatives=False), "svdf_rank_eval_positions"),
                       (lambda: t.rank_eval(USERS, *POS, sampled=None), "svdf_rank_eval"),
                       (lambda: g.rank_positions(USERS, *POS, feedback=FB, sampled=None), "svdf_rank_eval_positions_fb"),
                       (lambda: g.rank_eval(USERS, *POS, feedback=FB, sampled=None), "svdf_rank_eval_fb"),
                       (lambda: t.rank_positions(None, *POS, lines=UL, sampled=None), "svdf_rank_eval_positions_lines"),
                       (lambda: t.rank_eval(None, *POS, lines=UL, sampled=None), "svdf_rank_eval_lines"),
                       (lambda: t.rank_positions(USERS, *POS, candidates=cand, sampled=None), "svdf_rank_eval_positions_cand"),
                       (lambda: t.rank_eval(None, *POS, lines=UL, candidates=cand, sampled=None), "svdf_rank_eval_cand"),
                       (lambda: t.rank_topn(USERS, 5), "svdf_rank_topn"),
                       (lambda: t.rank_positions(USERS, *POS, *BAN, sampled=(2, 5)), "svdf_rank_eval_positions_sampled"),
                       (lambda: g.rank_positions(None, *POS, lines=UL, feedback=FB, sampled=(2, 5), return_negatives=True), "svdf_rank_eval_positions_sampled"),
                       (lambda: g.rank_eval(USERS, *POS, *BAN, feedback=FB, sampled=(2, 5)), "svdf_rank_eval_sampled")):
        del t.lib.names[:], g.lib.names[:]
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call()
        assert t.lib.names + g.lib.names == [want]

"""Live-model ranking against negatives drawn on the GPU (svdf_rank_eval*_sampled, svdf_k_ranknegs.hip).  The drawn ids must be
the published rule's (the host export svdf_rank_negatives and the numpy statement tests/rank_negs_rule.py); every other output must equal the
_cand call given each section's drawn row as its list, the numpy ranking rule of tests/test_rank_cand.py over that set, and the full-catalogue
call under the complement of the set as bans.  The models and sections are those of tests/test_gpu_rank_cand.py (trained once, shared)."""
import numpy as np
import pytest

import svdfeature_amd as sa
from rank_negs_rule import draws, rule_negatives
from test_gpu_rank_cand import KINDS, KS, assert_both_same, ban_both, cand_both, section_args, trained
from test_gpu_rank_lines import lines_trainer
from test_rank_cand import NI, NOPOS, NS, SAME_USER, complement, rule_cand_positions
from test_rank_feedback import ptr_of
from test_rank_negs import NEGS, make_bans

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTERS = (38, 40, 41, 42, 43)
SEED = 12345


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("rank_negs")


def sampled(t, c, num_neg, seed=SEED, bans=None, negatives=True):
    users, kw = section_args(c)
    return t.rank_positions(users, c["pos_ptr"], c["pos_item"], *(bans or c["neg_bans"]), sampled=(num_neg, seed), return_negatives=negatives, **kw)


def lists_of(neg):
    """each section's drawn row as its candidate list (a section without positives: an empty one)"""
    rows = [r[r >= 0].astype(np.uint32) for r in neg]
    return ptr_of(rows), np.concatenate(rows)


def with_bans(tmp, kind, k):
    c = trained(tmp, kind, k)
    if "neg_bans" not in c:
        c["neg_bans"] = make_bans(c["pos_ptr"], c["pos_item"], NI, seed=k + 11)
    return c


def check_against_every_route(c, got, num_neg, seed=SEED, bans=None):
    """got = (position, tied, ranked, nan, neg) of a sampled call on the sections of c"""
    t = c["t"]
    users, kw = section_args(c)
    ban_ptr, ban_item = bans or c["neg_bans"]
    position, tied, ranked, nan, neg = got
    want_neg = sa.rank_negatives(NI, c["pos_ptr"], c["pos_item"], ban_ptr, ban_item, num_neg, seed)
    np.testing.assert_array_equal(neg, want_neg)
    np.testing.assert_array_equal(neg, rule_negatives(NI, c["pos_ptr"], c["pos_item"], ban_ptr, ban_item, num_neg, seed))
    has_pos = np.diff(c["pos_ptr"]) > 0
    np.testing.assert_array_equal(ranked, np.where(has_pos, np.diff(c["pos_ptr"]) + num_neg, num_neg))
    cand = lists_of(neg)
    listed = t.rank_positions(users, c["pos_ptr"], c["pos_item"], candidates=cand, **kw)
    for a, b in zip((position, tied, nan), (listed[0], listed[1], listed[3])):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ranked[has_pos], listed[2][has_pos])
    want = rule_cand_positions(c["rows"], c["W"], c["bias"], c["pos_ptr"], c["pos_item"], *cand)
    for a, b in zip((position, tied, nan), (want[0], want[1], want[3])):
        np.testing.assert_array_equal(a, b)
    old = t.rank_positions(users, c["pos_ptr"], c["pos_item"], *complement(NI, *cand, c["pos_ptr"], c["pos_item"]), **kw)
    for a, b in zip((position, tied, nan), (old[0], old[1], old[3])):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_equals_every_route(tmp, kind, k):
    """40 sections over 1 200 items, 99 negatives: bans of 0 .. 190 ids with duplicates, a ban that would be drawn first, a section without
    positives, user 7 in three sections.  The drawn ids are the rule's; positions, `tied`, `ranked` and `nan` equal the _cand call on the drawn
    rows, the numpy ranking rule and the full-catalogue call under complement bans; the counters count; the older calls answer afterwards what
    they answered before"""
    c = with_bans(tmp, kind, k)
    t = c["t"]
    users, kw = section_args(c)
    ban_ptr, ban_item = c["neg_bans"]
    first = [int(draws(SEED, s, 0, NI)) for s in range(NS)]
    assert sum(first[s] in ban_item[ban_ptr[s]:ban_ptr[s + 1]] for s in range(NS)) >= 3
    before = [t.counter(w) for w in COUNTERS]
    got = sampled(t, c, 99)
    ranked_sections = NS - 1
    assert [t.counter(w) - b for w, b in zip(COUNTERS, before)] == [ranked_sections, ranked_sections if c["fmt"] == 1 else 0,
                                                                     ranked_sections if kind == "lines" else 0, 0, ranked_sections]
    check_against_every_route(c, got, 99)
    position, tied, ranked, nan, neg = got
    assert not nan.any() and (neg[NOPOS] == -1).all() and (position >= 0).all() and ranked[NOPOS] == 99
    assert all(first[s] not in neg[s] for s in range(NS) if first[s] in ban_item[ban_ptr[s]:ban_ptr[s + 1]])
    a, b, d = (neg[s] for s in SAME_USER)                       # one user in three sections: three lists
    assert (a != b).any() and (a != d).any() and (b != d).any()
    # without the negatives: the same four arrays
    four = sampled(t, c, 99, negatives=False)
    assert len(four) == 4
    for x, y in zip(four, got[:4]):
        np.testing.assert_array_equal(x, y)
    # either form of the score kernel
    for form in (1, 2):
        t.set_knob("rank_cand_form", form)
        again = sampled(t, c, 99)
        t.set_knob("rank_cand_form", 0)
        for x, y in zip(again, got):
            np.testing.assert_array_equal(x, y)
    m = t.rank_eval(users, c["pos_ptr"], c["pos_item"], ban_ptr, ban_item, at=(1, 10), sampled=(99, SEED), **kw)
    assert m == sa.rank_metrics(c["pos_ptr"], position, ranked=ranked, nan=nan, at=(1, 10)) and m["ninst"] == NS - 1
    # a full-catalogue call and a _cand call on the same trainer, after the sampled calls: the bits they gave before any of them
    assert_both_same(ban_both(t, c, c["N"]), c["old"])
    assert_both_same(cand_both(t, c, c["N"]), c["old"])


@pytest.mark.parametrize("num_neg", [n for n in NEGS if n != 99])
def test_every_round_count_on_one_model(tmp, num_neg):
    """1, 63, 64, 65 and 500 negatives: less than a round of 64 draws, a round that fills exactly, one more, and many rounds"""
    c = with_bans(tmp, "users", 64)
    check_against_every_route(c, sampled(c["t"], c, num_neg, seed=77), num_neg, seed=77)


def test_the_pinned_section_on_the_device(tmp):
    """seed 12345, section 7 excluding {25, 303} (its positive and a ban given twice): 1196 is drawn twice, 25 and 303 are skipped"""
    c = with_bans(tmp, "users", 64)
    S = 9
    pos = [np.array([1199 - s], np.uint32) for s in range(S)]
    pos[7] = np.array([25], np.uint32)
    ban = [np.zeros(0, np.uint32)] * 7 + [np.array([303, 303], np.uint32), np.zeros(0, np.uint32)]
    cc = dict(c, users=c["users"][:S], pos_ptr=ptr_of(pos), pos_item=np.concatenate(pos))
    neg = sampled(c["t"], cc, 5, bans=(ptr_of(ban), np.concatenate(ban)))[4]
    assert neg[7].tolist() == [1196, 504, 615, 588, 726] and neg[0].tolist() == [18, 601, 213, 846, 111]
    neg = sampled(c["t"], cc, 8, bans=(np.zeros(S + 1, np.int64), np.zeros(0, np.uint32)))[4]      # without the ban 303 is drawn
    assert neg[7][:6].tolist() == [1196, 303, 504, 615, 588, 726] and 25 not in neg[7]


def test_a_section_that_just_passes_the_availability_rule(tmp):
    """1 000 of 1 200 ids excluded (999 bans and the positive) and 100 negatives: avail = 200 = 2 * num_neg, about 13 rounds of 64 draws; one
    ban more is refused on the host"""
    c = with_bans(tmp, "users", 64)
    t = c["t"]
    ids = np.random.default_rng(5).permutation(NI).astype(np.uint32)
    S = 3
    pos = [ids[:1], ids[:1], ids[:1]]
    ban = [ids[1:1000], ids[1:40], ids[1:1000][::-1]]
    cc = dict(c, users=c["users"][:S], pos_ptr=ptr_of(pos), pos_item=np.concatenate(pos), rows=c["rows"][:S])
    bans = (ptr_of(ban), np.concatenate(ban))
    got = sampled(t, cc, 100, bans=bans)
    check_against_every_route(cc, got, 100, bans=bans)
    assert not np.isin(got[4][0], ids[:1000]).any() and len(np.unique(got[4][0])) == 100
    launches = t.counter(1)
    ban[2] = ids[1:1001]
    with pytest.raises(sa.SvdfError, match="rank_eval: section 2 leaves 199 items to draw 100 negatives from 1200; list its candidates instead"):
        sampled(t, cc, 100, bans=(ptr_of(ban), np.concatenate(ban)))
    assert t.counter(1) == launches


def test_the_largest_table():
    """9 000 items, three sections, 4 096 negatives each: the table of seen ids takes its 8 192 slots (32 KiB of LDS)"""
    ni, k, S = 9000, 16, 3
    t = lines_trainer(50, ni, k, 0)
    rng = np.random.default_rng(9)
    W = t.view("W_item").copy()
    W[:] = rng.standard_normal(W.shape).astype(F32)
    t.set_view("W_item", W)
    users = np.array([3, 4, 3], np.uint32)
    pos_ptr, pos_item = np.array([0, 2, 2, 3], np.int64), np.array([17, 8999, 0], np.uint32)
    ban_item = np.setdiff1d(rng.permutation(ni)[:300], pos_item).astype(np.uint32)      # all in section 0
    ban_ptr = np.array([0] + [len(ban_item)] * 3, np.int64)
    position, tied, ranked, nan, neg = t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item, sampled=(4096, 1), return_negatives=True)
    np.testing.assert_array_equal(neg, sa.rank_negatives(ni, pos_ptr, pos_item, ban_ptr, ban_item, 4096, 1))
    np.testing.assert_array_equal(neg, rule_negatives(ni, pos_ptr, pos_item, ban_ptr, ban_item, 4096, 1))
    assert ranked.tolist() == [4098, 4096, 4097] and (neg[1] == -1).all() and not nan.any()
    listed = t.rank_positions(users, pos_ptr, pos_item, candidates=lists_of(neg))
    np.testing.assert_array_equal(position, listed[0])
    np.testing.assert_array_equal(tied, listed[1])
    rows, W, bias = t.view("W_user")[users], t.view("W_item").copy(), t.view("i_bias").copy()
    want = rule_cand_positions(rows, W, bias, pos_ptr, pos_item, *lists_of(neg))
    np.testing.assert_array_equal(position, want[0])


@pytest.mark.parametrize("k", [64, 320])
def test_a_nan_row_flags_only_the_sections_that_draw_it(tmp, k):
    """item `bad` gets a NaN row: it lies in the drawn sets of some sections and outside the others' (read from neg_out)"""
    c = with_bans(tmp, "users", k)
    t = c["t"]
    clean = sampled(t, c, 99)
    neg = clean[4]
    bad = int(neg[3][1])
    in_set = np.array([bad in neg[s] or bad in c["pos_item"][c["pos_ptr"][s]:c["pos_ptr"][s + 1]] for s in range(NS)]).astype(np.int32)
    in_set[NOPOS] = 0
    assert 1 <= in_set.sum() < NS - 10 and in_set[3]
    W = t.view("W_item").copy()
    keep = W[bad].copy()
    W[bad, k // 2] = np.nan
    t.set_view("W_item", W)
    position, tied, ranked, nan, neg2 = sampled(t, c, 99)
    W[bad] = keep
    t.set_view("W_item", W)
    np.testing.assert_array_equal(nan, in_set)
    np.testing.assert_array_equal(neg2, neg)
    np.testing.assert_array_equal(ranked, clean[2])
    for s in range(NS):
        a, b = c["pos_ptr"][s], c["pos_ptr"][s + 1]
        if in_set[s]:
            assert (position[a:b] == -1).all() and (tied[a:b] == -1).all()
        else:
            np.testing.assert_array_equal(position[a:b], clean[0][a:b])
    for x, y in zip(sampled(t, c, 99), clean):                  # the model is what it was
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("kind, k", [("users", 64), ("lines", 128)])
def test_results_do_not_depend_on_the_pieces(tmp, kind, k):
    """rank_eval_budget lowered until the call takes several pieces: the stream of a section is that of its index in the CALL"""
    c = with_bans(tmp, kind, k)
    t = c["t"]
    want = sampled(t, c, 99)
    total = (NS - 1) * 99
    for budget in (1000, 300, 1):
        assert total >= 3 * budget
        before = [t.counter(w) for w in COUNTERS]
        launches = t.counter(1)
        t.set_knob("rank_eval_budget", budget)
        got = sampled(t, c, 99)
        t.set_knob("rank_eval_budget", 1 << 22)
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)
        assert t.counter(38) - before[0] == NS - 1 == t.counter(43) - before[4] and t.counter(42) == before[3]
        assert t.counter(1) - launches >= 3 * 3              # at least 3 pieces of three launches each


def test_nothing_is_launched_without_positives_or_after_a_refusal(tmp):
    c = with_bans(tmp, "users", 64)
    t = c["t"]
    before = [t.counter(w) for w in COUNTERS]
    launches = t.counter(1)
    with pytest.raises(sa.SvdfError, match="rank_eval: num_neg must be between 1 and 4096"):
        t.rank_positions([1, 2], [0, 1, 2], [5, 6], sampled=(0, 1))
    with pytest.raises(sa.SvdfError, match="each pos sample item can not occur in baned sample list"):
        t.rank_positions([1, 2], [0, 1, 2], [5, 6], [0, 0, 1], [6], sampled=(5, 1))
    with pytest.raises(sa.SvdfError, match="rank_eval: candidates and sampled exclude each other"):
        t.rank_positions([1, 2], [0, 1, 2], [5, 6], candidates=([0, 1, 2], [7, 8]), sampled=(5, 1))
    out = t.rank_positions([], [0], [], sampled=(5, 1), return_negatives=True)
    assert [len(x) for x in out] == [0] * 5 and out[4].shape == (0, 5)
    position, tied, ranked, nan, neg = t.rank_positions([1, 2], [0, 0, 0], [], [0, 1, 2], [4, 5], sampled=(5, 1), return_negatives=True)
    assert len(position) == 0 and ranked.tolist() == [5, 5] and nan.tolist() == [0, 0] and (neg == -1).all() and neg.shape == (2, 5)
    assert [t.counter(w) for w in COUNTERS] == before and t.counter(1) == launches

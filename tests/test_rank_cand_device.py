"""The device build of the _cand calls' sets (knobs rank_cand_build / rank_cand_build_form), the parts that need no GPU: the
knobs' legal values, the counters 58 .. 60, and the host refusals, which still come before "needs a GPU" with the device build asked for."""
import pytest

import svdfeature_amd as sa
from test_rank_cand import CAND, POS, USERS, calls
from test_rank_eval import host_trainer


def test_knobs_take_their_legal_values_and_the_counters_start_at_zero():
    t = host_trainer()
    assert [t.counter(w) for w in (58, 59, 60)] == [0, 0, 0]
    for name, legal, bad in (("rank_cand_build", (1, 0), (-1, 2)), ("rank_cand_build_form", (1, 2, 0), (-1, 3))):
        for v in legal:
            t.set_knob(name, v)
        for v in bad:
            with pytest.raises(sa.SvdfError, match=name + " must be"):
                t.set_knob(name, v)
    # a handle nobody has set a knob on takes today's path: the legal call reaches the device question with no counter moved
    with pytest.raises(sa.SvdfError, match="rank_eval needs a GPU"):
        t.rank_positions(USERS, *POS, candidates=CAND)
    assert [t.counter(w) for w in (58, 59, 60)] == [0, 0, 0]


@pytest.mark.parametrize("form", [0, 1, 2])
def test_host_refusals_still_come_before_the_device(form):
    t = host_trainer()
    t.set_knob("rank_cand_build", 1)
    t.set_knob("rank_cand_build_form", form)
    for j, who in enumerate(("rank_eval", "rank_eval", "rank_topn")):       # rank_positions, rank_eval, rank_topn
        with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
            calls(t, USERS, ([0, 3, 5], [1, 2, 2, 8, 30]))[j]()
        with pytest.raises(sa.SvdfError, match=who + ": cand_ptr must not decrease"):
            calls(t, USERS, ([0, 3, 2], [1, 2, 2, 8, 29]))[j]()
        with pytest.raises(sa.SvdfError, match=who + ": cand_item is missing"):
            calls(t, USERS, ([0, 3, 5], None))[j]()
        with pytest.raises(sa.SvdfError, match=who + " needs a GPU"):
            calls(t, USERS, CAND)[j]()
    # the positives' refusals, which the host build made while it built the sets: out of bound before repeated, section by section
    with pytest.raises(sa.SvdfError, match="rank_eval: a positive item is repeated inside a section"):
        t.rank_positions(USERS, [0, 2, 3], [5, 5, 7], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions(USERS, [0, 3, 4], [5, 5, 30, 7], candidates=CAND)
    with pytest.raises(sa.SvdfError, match="rank_eval: a positive item is repeated inside a section"):
        t.rank_positions(USERS, [0, 2, 3], [5, 5, 30], candidates=CAND)
    assert [t.counter(w) for w in (58, 59, 60, 42)] == [0, 0, 0, 0]

"""The checker of the window step on user-group (SVD++) blocks (tests/window_sim.py: step_blocks), pinned on the CPU (helpers and fixture:
tests/test_shared_hot_checker.py):
  * to what exists outside it: on blocks with one user entry per row it is oracle.update_block_stale plus the window's add, and on blocks with
    empty feedback lists it is step_rows on the same rows, lanes included -- bit for bit; sub-steps of 1 on a row that alone links its
    window's blocks are the port's sequential update_block at 1e-5;
  * lane against walk: ONE sub-step that holds every slot (hot_over / ihot_over = 0) is the plain step_blocks, bit for bit;
  * every checker run is the recorded one (tests/golden/window_checkers.npz), both lanes on spans with feedback among them."""
import numpy as np
import pytest

import cases
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT
from test_shared_hot_checker import _same, case, run_case

BP, BS, BI, BF = 30, 6, 25, 25           # private users, shared users, items, feedback ids
SVDPP_EXTRA = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]


def _bconf(k, extra=(), ni=BI):
    return cases.conf_with(cases.BASICMF_CONF, num_user=BP + BS, num_item=ni, num_factor=k, num_ufeedback=BF, learning_rate="0.01") + SVDPP_EXTRA + list(extra)


P_BLOCK_STALE = [(6, ()), (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01"))), (5, (("no_user_bias", "1"),))]


@case(*P_BLOCK_STALE)
def one_user_entry_per_row_is_the_block_checker_plus_the_windows_add(S, tmp, k, extra):
    rng = np.random.default_rng(k)
    blocks = S.shared_blocks(rng, 40, BP, BS, BI, BI, max_shared=0, split_every=3)
    ba = BlockArrays.from_blocks(blocks)
    a = S.make_oracle(_bconf(k, extra), user_group=True)
    S.simulate_blocks(a, ba, BP + BS, 3, 2, user_bias=dict(extra).get("no_user_bias") != "1")   # B = num_user: no id is shared
    return dict(a=a, blocks=blocks, ba=ba)


@pytest.mark.parametrize("k,extra", P_BLOCK_STALE)
def test_one_user_entry_per_row_is_the_block_checker_plus_the_windows_add(request, k, extra):
    out = run_case(request, (k, extra))
    blocks, ba = out["blocks"], out["ba"]
    b = ws.make_oracle(_bconf(k, extra), user_group=True)
    for _ in range(2):
        for b0, b1 in ws.block_cuts(ba, 3):
            delta = b.stale_delta_zero()
            for blk in blocks[b0:b1]:
                delta = b.update_block_stale(blk, delta)
            for name, d in zip(("W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias"), delta):
                v = b.view(name)
                if v is not None and v.size:
                    b.set_view(name, (v + d.reshape(v.shape)).astype(np.float32))
    assert len(ws.spans(blocks)) < len(blocks)   # (START..END spans among them)
    _same(out["a"], b, ("W_user", "u_bias", "W_item", "i_bias", "W_ufeedback", "ufeedback_bias"))


def _as_rows(S, ba, a, conf, W, **kw):
    """step_rows over the rows of the block windows, on a trainer without feedback that starts from a's model (the two formats draw their
    initial models differently)"""
    b = S.make_oracle(cases.conf_with(conf, num_ufeedback=0))
    for name in S.SHARED:
        b.set_view(name, a.view(name))
    return b, lambda: [S.step_rows(b, ba.rows().slice_rows(int(ba.block_row_ptr[b0]), int(ba.block_row_ptr[b1])), BP, **kw)
                       for _ in range(2) for b0, b1 in S.block_cuts(ba, W)]


P_NO_FEEDBACK = [(6, False), (8, "all")]


@case(*P_NO_FEEDBACK)
def empty_feedback_lists_are_the_shared_user_checker(S, tmp, k, uvals):
    rng = np.random.default_rng(20 + k)
    blocks = S.shared_blocks(rng, 40, BP, BS, BI, BI, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=3)
    assert all(b.num_ufeedback == 0 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _bconf(k)
    a = S.make_oracle(conf, user_group=True)
    b, walk = _as_rows(S, ba, a, conf, 3)
    S.simulate_blocks(a, ba, BP, 3, 2)
    walk()
    return dict(a=a, b=b)


@pytest.mark.parametrize("k,uvals", P_NO_FEEDBACK)
def test_empty_feedback_lists_are_the_shared_user_checker(request, k, uvals):
    out = run_case(request, (k, uvals))
    _same(out["a"], out["b"])


P_BLOCK_USER_LANE = [(6, (), dict(max_shared=3, uvals=True)),
                     (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(max_shared=3, uvals="all", per_row=True)),
                     (5, (("no_user_bias", "1"),), dict(min_shared=1, max_shared=4))]


@case(*P_BLOCK_USER_LANE)
def one_user_sub_step_holding_every_slot_is_the_block_shared_checker(S, tmp, k, extra, opts):
    rng = np.random.default_rng(k)
    blocks = S.shared_blocks(rng, 40, BP, BS, BI, BI, split_every=3, **opts)
    ba = BlockArrays.from_blocks(blocks)
    conf = _bconf(k, extra)
    ub = dict(extra).get("no_user_bias") != "1"
    a, b = S.make_oracle(conf, user_group=True), S.make_oracle(conf, user_group=True)
    nhot = S.simulate_blocks(a, ba, BP, 3, 2, sub=ba.num_row + 1, user_bias=ub, hot_over=0)
    S.simulate_blocks(b, ba, BP, 3, 2, user_bias=ub)
    return dict(a=a, b=b, nhot=nhot)


@pytest.mark.parametrize("k,extra,opts", P_BLOCK_USER_LANE)
def test_one_user_sub_step_holding_every_slot_is_the_block_shared_checker(request, k, extra, opts):
    out = run_case(request, (k, extra, opts))
    assert out["nhot"][0] > 0 and out["nhot"][1] == 0
    _same(out["a"], out["b"], ws.VIEWS)


P_BLOCK_AS_SHARED_HOT = [(6, False, 2), (8, "all", 3)]


@case(*P_BLOCK_AS_SHARED_HOT)
def one_row_blocks_with_empty_feedback_lists_are_the_shared_hot_checker(S, tmp, k, uvals, sub):
    rng = np.random.default_rng(20 + k)
    blocks = S.shared_blocks(rng, 90, BP, BS, BI, BI, max_rows=1, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=0)
    assert all(b.num_ufeedback == 0 and b.data.num_row == 1 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _bconf(k)
    a = S.make_oracle(conf, user_group=True)
    b, walk = _as_rows(S, ba, a, conf, 3, sub=sub)
    nhot = S.simulate_blocks(a, ba, BP, 3, 2, sub=sub)
    walk()
    return dict(a=a, b=b, nhot=nhot)


@pytest.mark.parametrize("k,uvals,sub", P_BLOCK_AS_SHARED_HOT)
def test_one_row_blocks_with_empty_feedback_lists_are_the_shared_hot_checker(request, k, uvals, sub):
    out = run_case(request, (k, uvals, sub))
    assert out["nhot"][0] > 0
    _same(out["a"], out["b"])


def _linked_blocks(user_lane):
    """a window whose private users, (other) items and feedback ids occur once: only the hot row links its blocks.  The hot item's blocks
    have two rows, the hot one first or second: the slot starts from a span state (private row, tmp_ufeedback) that has moved"""
    nb, blocks = 10, []
    for j in range(nb):
        if user_lane:
            rows = [(float(1 + j % 5), [], [(j, 1.0), (BP + 2, 0.5)] if j % 2 else [(BP + 2, 0.5), (j, 1.0)], [(j, 1.0)])]
        else:
            rows = [(float(1 + j % 5), [], [(j, 1.0)], [(1 + j, 1.0)]), (float(1 + (j + 2) % 5), [], [(j, 1.0)], [(0, 1.0)])][::-1 if j % 2 else 1]
        fbi = np.array([2 * j, 2 * j + 1], np.uint32)
        blocks.append(PlusBlock(fbi, np.full(2, 2 ** -0.5, np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    assert nb + 1 <= 12 and 2 * nb <= BF
    return blocks


@case((6,), (8,))
def sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(S, tmp, k):
    a = S.make_oracle(_bconf(k), user_group=True)
    return dict(a=a, nhot=S.step_blocks(a, _linked_blocks(True), BP, sub=1))


@pytest.mark.parametrize("k", [6, 8])
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(request, k):
    """sub-steps of 1 ARE the sequential update_block for the row that alone links the window's blocks -- up to the order of roundings
    (new - current + current), 1e-5 like the sub-steps of one on rows"""
    out = run_case(request, (k,))
    assert out["nhot"] == (1, 0)
    b, hot = ws.make_oracle(_bconf(k), user_group=True), BP + 2
    for blk in _linked_blocks(True):
        b.update_block(blk)
    for name in ("W_user", "u_bias"):
        x, y = out["a"].view(name), b.view(name)
        assert not np.array_equal(x[hot], ws.make_oracle(_bconf(k), user_group=True).view(name)[hot])   # it moved
        assert np.allclose(x[hot], y[hot], rtol=0, atol=1e-5), name


P_BLOCK_ITEM_LANE = [(6, (), dict(max_shared=0)),
                     (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(max_shared=3, uvals="all", per_row=True)),
                     (5, (("no_user_bias", "1"),), dict(min_shared=1, max_shared=4))]


@case(*P_BLOCK_ITEM_LANE)
def one_sub_step_holding_every_slot_is_the_block_shared_checker(S, tmp, k, extra, opts):
    rng = np.random.default_rng(k)
    blocks = S.shared_blocks(rng, 40, BP, BS, 9, BF, split_every=3, **opts)
    ba = BlockArrays.from_blocks(blocks)
    conf = _bconf(k, extra, ni=9)
    ub = dict(extra).get("no_user_bias") != "1"
    a, b = S.make_oracle(conf, user_group=True), S.make_oracle(conf, user_group=True)
    nhot = S.simulate_blocks(a, ba, BP, 3, 2, isub=ba.num_row + 1, user_bias=ub, ihot_over=0)
    S.simulate_blocks(b, ba, BP, 3, 2, user_bias=ub)
    return dict(a=a, b=b, nhot=nhot)


@pytest.mark.parametrize("k,extra,opts", P_BLOCK_ITEM_LANE)
def test_one_sub_step_holding_every_slot_is_the_block_shared_checker(request, k, extra, opts):
    out = run_case(request, (k, extra, opts))
    nu, ni = out["nhot"]
    assert ni > 0 and nu == 0
    _same(out["a"], out["b"], ws.VIEWS)


P_BLOCK_AS_ITEM_HOT = [(6, False, 2, 0), (8, "all", 3, 0), (8, True, 3, 2)]


@case(*P_BLOCK_AS_ITEM_HOT)
def one_row_blocks_with_empty_feedback_lists_are_the_item_hot_checker(S, tmp, k, uvals, isub, sub):
    rng = np.random.default_rng(20 + k)
    blocks = S.shared_blocks(rng, 90, BP, BS, 9, BF, max_rows=1, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=0)
    assert all(b.num_ufeedback == 0 and b.data.num_row == 1 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _bconf(k, ni=9)
    a = S.make_oracle(conf, user_group=True)
    b, walk = _as_rows(S, ba, a, conf, 3, isub=isub, sub=sub)
    nhot = S.simulate_blocks(a, ba, BP, 3, 2, isub=isub, sub=sub)
    walk()
    return dict(a=a, b=b, nhot=nhot)


@pytest.mark.parametrize("k,uvals,isub,sub", P_BLOCK_AS_ITEM_HOT)
def test_one_row_blocks_with_empty_feedback_lists_are_the_item_hot_checker(request, k, uvals, isub, sub):
    out = run_case(request, (k, uvals, isub, sub))
    nu, ni = out["nhot"]
    assert ni > 0 and (nu > 0) == (sub > 0)
    _same(out["a"], out["b"])


@case((6,), (8,))
def sub_steps_of_one_move_the_hot_item_like_the_sequential_pass(S, tmp, k):
    a = S.make_oracle(_bconf(k, ni=12), user_group=True)
    return dict(a=a, nhot=S.step_blocks(a, _linked_blocks(False), BP + BS, isub=1))


@pytest.mark.parametrize("k", [6, 8])
def test_sub_steps_of_one_move_the_hot_item_like_the_sequential_pass(request, k):
    """sub-steps of 1 ARE the sequential update_block for the item that alone links the window's blocks -- up to the order of roundings
    (new - current + current), 1e-5 like the hot user row's"""
    out = run_case(request, (k,))
    assert out["nhot"] == (0, 1)
    b, hot = ws.make_oracle(_bconf(k, ni=12), user_group=True), 0
    for blk in _linked_blocks(False):
        b.update_block(blk)
    for name in ("W_item", "i_bias"):
        x, y = out["a"].view(name), b.view(name)
        assert not np.array_equal(x[hot], ws.make_oracle(_bconf(k, ni=12), user_group=True).view(name)[hot])   # it moved
        assert np.allclose(x[hot], y[hot], rtol=0, atol=1e-5), name


P_BLOCK_BOTH = [(6, (), 2, 3), (7, (("no_user_bias", "1"), ("scale_lr_ufeedback", "0.5")), 1, 2)]


@case(*P_BLOCK_BOTH)
def both_lanes_on_spans_with_feedback_are_the_recorded_block_item_hot_checker(S, tmp, k, extra, sub, isub):
    rng = np.random.default_rng(40 + k)
    blocks = S.shared_blocks(rng, 30, BP, BS, 9, BF, split_every=3, min_shared=1, max_shared=3, uvals=True)
    ba = BlockArrays.from_blocks(blocks)
    a = S.make_oracle(_bconf(k, extra, ni=9), user_group=True)
    nhot = S.simulate_blocks(a, ba, BP, 2, 2, sub=sub, isub=isub, user_bias=dict(extra).get("no_user_bias") != "1")
    return dict(a=a, nhot=nhot, blocks=blocks, ba=ba)


@pytest.mark.parametrize("k,extra,sub,isub", P_BLOCK_BOTH)
def test_both_lanes_on_spans_with_feedback_are_the_recorded_block_item_hot_checker(request, k, extra, sub, isub):
    """DEFAULT blocks and START..END spans with feedback lists, hot user rows and hot item rows in one window, data rows with two hot entries"""
    out = run_case(request, (k, extra, sub, isub))
    blocks, ba = out["blocks"], out["ba"]
    assert out["nhot"][0] > 0 and out["nhot"][1] > 0
    assert any(b.num_ufeedback for b in blocks) and len(ws.spans(blocks)) < len(blocks)
    two = 0
    for b0, b1 in ws.block_cuts(ba, 2):
        uhot = {s for s, c in ws.slot_counts(blocks[b0:b1], BP).items() if c > sub}
        ihot = {i for i, c in ws.block_item_slot_counts(blocks[b0:b1]).items() if c > isub}
        for _, _, d in ws.spans(blocks[b0:b1]):
            for r in range(d.num_row):
                _, ng, nu, _, idx, _ = d.row(r)
                two += sum(int(x) in uhot for x in idx[ng:ng + nu]) + sum(int(x) in ihot for x in idx[ng + nu:]) >= 2
    assert two > 0

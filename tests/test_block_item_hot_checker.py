"""tests/block_item_hot_sim.py (the checker of the ordered sub-steps for hot item rows of SVD++ blocks, knob window_block_item_sub, DESIGN.md
section 6u) pinned, on the CPU, to the checkers that exist: with every item row sent through the lane in ONE sub-step it must be
block_shared_sim.window_step bit for bit; on one-row blocks with empty feedback lists it must be item_hot_sim.window_step on the same rows bit
for bit (hot shared user rows next to the hot items included); and with sub-steps of 1 a hot item whose window holds every user, other item and
feedback id once moves like the reference's sequential update_block."""
import numpy as np
import pytest

import block_item_hot_sim as sim
import block_shared_sim
import cases
import item_hot_sim
import shared_user_sim
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT

SVDPP_EXTRA = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
NP, NS, NI, NF = 30, 6, 9, 25


def _conf(k, extra=(), ni=NI, **kw):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=ni, num_factor=k, num_ufeedback=NF, learning_rate="0.01", **kw) + SVDPP_EXTRA + list(extra)


def _same(a, b, names):
    for name in names:
        x, y = a.view(name), b.view(name)
        if x is None or x.size == 0:
            continue
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


@pytest.mark.parametrize("k,extra,opts", [
    (6, (), dict(max_shared=0)),
    (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(max_shared=3, uvals="all", per_row=True)),
    (5, (("no_user_bias", "1"),), dict(min_shared=1, max_shared=4)),
])
def test_one_sub_step_holding_every_slot_is_the_block_shared_checker(k, extra, opts):
    rng = np.random.default_rng(k)
    blocks = sim.shared_blocks(rng, 40, NP, NS, NI, NF, split_every=3, **opts)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k, extra)
    ub = dict(extra).get("no_user_bias") != "1"
    a, b = sim.make_oracle(conf), sim.make_oracle(conf)
    nu, ni = sim.simulate(a, ba, NP, 3, 2, isub=ba.num_row + 1, user_bias=ub, ihot_over=0)
    assert ni > 0 and nu == 0
    block_shared_sim.simulate(b, ba, NP, 3, 2, user_bias=ub)
    _same(a, b, sim.VIEWS)


@pytest.mark.parametrize("k,uvals,isub,sub", [(6, False, 2, 0), (8, "all", 3, 0), (8, True, 3, 2)])
def test_one_row_blocks_with_empty_feedback_lists_are_the_item_hot_checker(k, uvals, isub, sub):
    rng = np.random.default_rng(20 + k)
    blocks = sim.shared_blocks(rng, 90, NP, NS, NI, NF, max_rows=1, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=0)
    assert all(b.num_ufeedback == 0 and b.data.num_row == 1 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k)
    a = sim.make_oracle(conf)
    b = shared_user_sim.make_oracle(cases.conf_with(conf, num_ufeedback=0))
    for name in shared_user_sim.SHARED:   # the two formats draw their initial models differently: start from one
        b.set_view(name, a.view(name))
    W = 3
    nu, ni = sim.simulate(a, ba, NP, W, 2, isub=isub, sub=sub)
    assert ni > 0 and (nu > 0) == (sub > 0)
    rows = ba.rows()
    for _ in range(2):
        for b0, b1 in sim.window_cuts(ba, W):
            item_hot_sim.window_step(b, rows.slice_rows(int(ba.block_row_ptr[b0]), int(ba.block_row_ptr[b1])), NP, isub, sub)
    _same(a, b, shared_user_sim.SHARED)


@pytest.mark.parametrize("k", [6, 8])
def test_sub_steps_of_one_move_the_hot_item_like_the_sequential_pass(k):
    """a window whose users, other items and feedback ids occur once: only the hot item links its blocks, so sub-steps of 1 ARE the sequential
    update_block for that row -- up to the order of roundings (new - current + current), 1e-5 like tests/test_block_hot_checker.py.  Every block
    has two rows, the hot one first or second: the slot starts from a span state (private row, tmp_ufeedback) that has moved"""
    nb, hot, ni = 10, 0, 12
    blocks = []
    for j in range(nb):
        rows = [(float(1 + j % 5), [], [(j, 1.0)], [(1 + j, 1.0)]), (float(1 + (j + 2) % 5), [], [(j, 1.0)], [(hot, 1.0)])]
        fbi = np.array([2 * j, 2 * j + 1], np.uint32)
        blocks.append(PlusBlock(fbi, np.full(2, 2 ** -0.5, np.float32), CSRData.from_rows(rows[::-1] if j % 2 else rows), TAG_DEFAULT))
    assert nb + 1 <= ni and 2 * nb <= NF
    conf = _conf(k, ni=ni)
    a, b = sim.make_oracle(conf), sim.make_oracle(conf)
    assert sim.window_step(a, blocks, NP + NS, 1) == (0, 1)
    for blk in blocks:
        b.update_block(blk)
    for name in ("W_item", "i_bias"):
        x, y = a.view(name), b.view(name)
        assert not np.array_equal(x[hot], block_shared_sim.make_oracle(conf).view(name)[hot])   # it moved
        assert np.allclose(x[hot], y[hot], rtol=0, atol=1e-5), name

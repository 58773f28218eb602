"""tests/block_hot_sim.py (the checker of the ordered sub-steps for hot shared user rows of SVD++ blocks, knob window_block_sub)
pinned, on the CPU, to the checkers that exist: with every shared row sent through the lane in ONE sub-step it must be
block_shared_sim.window_step bit for bit; on one-row blocks with empty feedback lists it must be shared_hot_sim.window_step on the same rows bit
for bit; and with sub-steps of 1 a hot row whose window holds every private user, item and feedback id once moves like the reference's
sequential update_block."""
import numpy as np
import pytest

import block_hot_sim as sim
import block_shared_sim
import cases
import shared_hot_sim
import shared_user_sim
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT

SVDPP_EXTRA = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
NP, NS, NI = 30, 6, 25


def _conf(k, extra=(), **kw):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_factor=k, num_ufeedback=NI, learning_rate="0.01", **kw) + SVDPP_EXTRA + list(extra)


def _same(a, b, names):
    for name in names:
        x, y = a.view(name), b.view(name)
        if x is None or x.size == 0:
            continue
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


@pytest.mark.parametrize("k,extra,opts", [
    (6, (), dict(max_shared=3, uvals=True)),
    (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01")), dict(max_shared=3, uvals="all", per_row=True)),
    (5, (("no_user_bias", "1"),), dict(min_shared=1, max_shared=4)),
])
def test_one_sub_step_holding_every_slot_is_the_block_shared_checker(k, extra, opts):
    rng = np.random.default_rng(k)
    blocks = sim.shared_blocks(rng, 40, NP, NS, NI, NI, split_every=3, **opts)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k, extra)
    ub = dict(extra).get("no_user_bias") != "1"
    a, b = sim.make_oracle(conf), sim.make_oracle(conf)
    nhot = sim.simulate(a, ba, NP, 3, 2, sub=ba.num_row + 1, user_bias=ub, hot_over=0)
    assert nhot > 0
    block_shared_sim.simulate(b, ba, NP, 3, 2, user_bias=ub)
    _same(a, b, sim.VIEWS)


@pytest.mark.parametrize("k,uvals,sub", [(6, False, 2), (8, "all", 3)])
def test_one_row_blocks_with_empty_feedback_lists_are_the_shared_hot_checker(k, uvals, sub):
    rng = np.random.default_rng(20 + k)
    blocks = sim.shared_blocks(rng, 90, NP, NS, NI, NI, max_rows=1, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=0)
    assert all(b.num_ufeedback == 0 and b.data.num_row == 1 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k)
    a = sim.make_oracle(conf)
    b = shared_user_sim.make_oracle(cases.conf_with(conf, num_ufeedback=0))
    for name in shared_user_sim.SHARED:   # the two formats draw their initial models differently: start from one
        b.set_view(name, a.view(name))
    W = 3
    assert sim.simulate(a, ba, NP, W, 2, sub=sub) > 0
    rows = ba.rows()
    for _ in range(2):
        for b0, b1 in sim.window_cuts(ba, W):
            shared_hot_sim.window_step(b, rows.slice_rows(int(ba.block_row_ptr[b0]), int(ba.block_row_ptr[b1])), NP, sub)
    _same(a, b, shared_user_sim.SHARED)


@pytest.mark.parametrize("k", [6, 8])
def test_sub_steps_of_one_move_the_hot_row_like_the_sequential_pass(k):
    """a window whose private users, items and feedback ids occur once: only the hot row links its blocks, so sub-steps of 1 ARE the sequential
    update_block for that row -- up to the order of roundings (new - current + current), 1e-5 like tests/test_shared_hot_checker.py"""
    nb = 10
    hot = NP + 2
    blocks = []
    for j in range(nb):
        rows = [(float(1 + j % 5), [], [(j, 1.0), (hot, 0.5)] if j % 2 else [(hot, 0.5), (j, 1.0)], [(j, 1.0)])]
        fbi = np.array([2 * j, 2 * j + 1], np.uint32)
        blocks.append(PlusBlock(fbi, np.full(2, 2 ** -0.5, np.float32), CSRData.from_rows(rows), TAG_DEFAULT))
    assert nb <= NI and 2 * nb <= NI
    conf = _conf(k)
    a, b = sim.make_oracle(conf), sim.make_oracle(conf)
    assert sim.window_step(a, blocks, NP, 1) == 1
    for blk in blocks:
        b.update_block(blk)
    for name in ("W_user", "u_bias"):
        x, y = a.view(name), b.view(name)
        assert not np.array_equal(x[hot], block_shared_sim.make_oracle(conf).view(name)[hot])   # it moved
        assert np.allclose(x[hot], y[hot], rtol=0, atol=1e-5), name

"""tests/block_shared_sim.py (the checker of the window step for SVD++ blocks with shared user ids) pinned, on the CPU, to the
two checkers that exist: on blocks with one user entry per row it must be oracle.update_block_stale plus the window's add (the checker of the
user-group window step, itself pinned to the compiled reference in tests/test_window_blocks.py), and on blocks with empty feedback lists it
must be shared_user_sim.window_step on the same rows (the checker of shared user rows on random-order trainers) -- bit for bit."""
import numpy as np
import pytest

import block_shared_sim as sim
import cases
import shared_user_sim
from svdfeature_amd import BlockArrays

SVDPP_EXTRA = [("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
NP, NS, NI = 30, 6, 25


def _conf(k, extra=()):
    return cases.conf_with(cases.BASICMF_CONF, num_user=NP + NS, num_item=NI, num_factor=k, num_ufeedback=NI, learning_rate="0.01") + SVDPP_EXTRA + list(extra)


def _same(a, b, names):
    for name in names:
        x, y = a.view(name), b.view(name)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name


@pytest.mark.parametrize("k,extra", [(6, ()), (9, (("scale_lr_ufeedback", "0.5"), ("wd_ufeedback_bias", "0.01"))), (5, (("no_user_bias", "1"),))])
def test_one_user_entry_per_row_is_the_block_checker_plus_the_windows_add(k, extra):
    rng = np.random.default_rng(k)
    blocks = sim.shared_blocks(rng, 40, NP, NS, NI, NI, max_shared=0, split_every=3)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k, extra)
    a, b = sim.make_oracle(conf), sim.make_oracle(conf)
    W = 3
    sim.simulate(a, ba, NP + NS, W, 2, user_bias=dict(extra).get("no_user_bias") != "1")   # B = num_user: no id is shared
    for _ in range(2):
        for b0, b1 in sim.window_cuts(ba, W):
            delta = b.stale_delta_zero()
            for blk in blocks[b0:b1]:
                delta = b.update_block_stale(blk, delta)
            for name, d in zip(("W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias"), delta):
                v = b.view(name)
                if v is not None and v.size:
                    b.set_view(name, (v + d.reshape(v.shape)).astype(np.float32))
    _same(a, b, ("W_user", "u_bias", "W_item", "i_bias", "W_ufeedback", "ufeedback_bias"))


@pytest.mark.parametrize("k,uvals", [(6, False), (8, "all")])
def test_empty_feedback_lists_are_the_shared_user_checker(k, uvals):
    rng = np.random.default_rng(20 + k)
    blocks = sim.shared_blocks(rng, 40, NP, NS, NI, NI, max_fb=0, max_shared=3, uvals=uvals, per_row=True, split_every=3)
    assert all(b.num_ufeedback == 0 for b in blocks)
    ba = BlockArrays.from_blocks(blocks)
    conf = _conf(k)
    a = sim.make_oracle(conf)
    b = shared_user_sim.make_oracle(cases.conf_with(conf, num_ufeedback=0))
    for name in shared_user_sim.SHARED:   # the two formats draw their initial models differently: start from one
        b.set_view(name, a.view(name))
    W = 3
    sim.simulate(a, ba, NP, W, 2)
    rows = ba.rows()
    for _ in range(2):
        for b0, b1 in sim.window_cuts(ba, W):
            shared_user_sim.window_step(b, rows.slice_rows(int(ba.block_row_ptr[b0]), int(ba.block_row_ptr[b1])), NP)
    _same(a, b, shared_user_sim.SHARED)

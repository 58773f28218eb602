"""The checker of the ordered sub-steps for hot items of rank pairs (knob `window_pair_sub`), CPU only.  The checker is
tests/window_sim.py on pair-shaped rows (tests/pair_hot_cases.py: check); here it is pinned on that shape:
  * ONE sub-step that holds every slot of every item (ihot_over = 0) is the plain window step -- window_sim.step_rows without sub-steps -- bit for bit;
  * sub-steps of s end elsewhere than the plain window step, and stay finite;
  * the Python restatement of the window rule that tests/test_gpu_pair_hot_window.py compares num_batches with, on hand-computed cases."""
import numpy as np
import pytest

import pair_hot_cases as ph
import window_rule as wr

# (k, active_type, reg_method, extra keys, sub-step)
CASES = [
    (1, 3, 0, (), 1),
    (7, 3, 1, (("wd_item_bias", "0.01"),), 3),
    (64, 3, 0, (("no_user_bias", "1"),), 5),
    (64, 0, 2, ph.ip_ranges(), 12),
    (128, 3, 3, (("no_user_bias", "1"),), 5),
]


def _pairs(k, s):
    rng = np.random.default_rng(300 + k + s)
    return ph.draw_pairs(rng, 300)


def _same(a, b):
    for name in ph.VIEWS:
        assert np.array_equal(a.view(name).view(np.uint32), b.view(name).view(np.uint32)), name


@pytest.fixture(scope="module")
def plain():
    """the plain window step of every case, computed once"""
    out = {}
    for k, active, reg, extra, s in CASES:
        u, p, q = _pairs(k, s)
        out[(k, s)] = ph.check(ph.conf(k, active, reg, extra), u, p, q, 4, 2, 0)
    return out


@pytest.mark.parametrize("k,active,reg,extra,s", CASES)
def test_one_sub_step_for_every_slot_is_the_plain_window_step(plain, k, active, reg, extra, s):
    u, p, q = _pairs(k, s)
    a = ph.check(ph.conf(k, active, reg, extra), u, p, q, 4, 2, 1000, ihot_over=0)
    _same(a, plain[(k, s)])


@pytest.mark.parametrize("k,active,reg,extra,s", CASES)
def test_sub_steps_differ_from_the_plain_window_step(plain, k, active, reg, extra, s):
    u, p, q = _pairs(k, s)
    f = ph.facts(p, q, 4, s)
    assert f["nhot"] >= 8 and f["two_hot"] > 0
    a = ph.check(ph.conf(k, active, reg, extra), u, p, q, 4, 2, s)
    assert all(np.isfinite(a.view(name)).all() for name in ph.VIEWS)
    b = plain[(k, s)]
    assert not np.array_equal(a.view("W_item")[:3], b.view("W_item")[:3])
    # what no lane touches -- a user's walk reads window-start item rows either way -- differs only through the item rows of LATER windows
    assert not np.array_equal(a.view("W_user"), b.view("W_user"))


def _pair_windows(counts, s=0, cap=0):
    """the window count of a pass of pairs whose items hold `counts` slots (both entries of a pair counted); s = 0: without the lane"""
    return wr.columns(sum(counts) // 2, counts, (s, cap))


def test_window_rule_on_hand_computed_cases():
    # every term below the bound at one window: min(c / 1, 5) = 5 for all three items, mean 5 <= 24
    assert _pair_windows([100, 10, 10], 5, 2048) == 1
    # the cap alone: ceil(5000 / 2048) = 3, and min(c / 3, 5) <= 5
    assert _pair_windows([5000, 10], 5, 2048) == 3
    assert _pair_windows([5000, 10], 5, 100) == 50
    # the mean binds: with s = 30 the hot item alone needs 5000 / W * 5000 + 100 / W <= 24 * 5010 = 120 240:
    #   W = 207: (24.1546 * 5000 + 0.483) / 5010 = 24.106 > 24;  W = 208: (24.0385 * 5000 + 0.481) / 5010 = 23.991 <= 24
    assert _pair_windows([5000, 10], 30, 2048) == 208
    # two equal items, s = 128: min(1000 / W, 128) <= 24 from W = 42 on (1000 / 41 = 24.39, 1000 / 42 = 23.81)
    assert _pair_windows([1000, 1000], 128, 2048) == 42
    # items without a slot change nothing; an empty pass is one window
    assert _pair_windows([0, 1000, 0, 1000], 128, 2048) == 42
    assert _pair_windows([0, 0], 8, 2048) == 1
    # the default rule, for comparison: max(sum c^2 / sum c, max c * 24 / 128) / 24, rounded up
    assert _pair_windows([5000, 10]) == 208     # 4990.04 / 24 = 207.9
    assert _pair_windows([1000, 1000]) == 42    # 1000 / 24 = 41.7
    assert _pair_windows([4000] + [100] * 60) == 70   # sum c^2 / sum c = 1660, / 24 = 69.2; the max term 4000 * 0.1875 / 24 = 31.25 does not bind

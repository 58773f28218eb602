"""The window rule of `amd:step = minibatch` on the CPU (svdf_wseq_rule.h; DESIGN.md sections 6, 6k, 6m, 6r): the engine's own functions -- reached
through the host-only probes svdf_window_rule / svdf_window_rule_as_cut / svdf_window_block_cuts, which call what the data-set builders call --
equal tests/window_rule.py, the one Python statement of the rule, exactly.  No GPU: the rule reads knob values and counts.  (On a GPU the same
Python is held against `num_batches` of real data sets: the window-orders, item-hot, shared-hot, block-hot, block-item-hot, pair-hot,
shared-user, side-table and block-shared tests.)"""
import numpy as np
import pytest

import svdfeature_amd as sa
import window_order_cases as woc
import window_rule as wr
from test_window_orders import HOT_MAX, HOT_SUB, N, NI, NU, PARENT_W, PER, PER_MAX, SEED

LANES = [wr.NO_LANE] + [(sub, cap) for sub in (3, 8, 24, 128) for cap in (64, 128, 2048)]   # (sub 0: no lane, whatever the cap)


def _zipf_counts(n, ids, s, seed):
    p = np.arange(1, ids + 1, dtype=np.float64) ** -s
    return np.random.default_rng(seed).multinomial(n, p / p.sum())


COLUMN_COUNTS = {
    "uniform": (20000, np.random.default_rng(1).multinomial(20000, np.full(200, 1 / 200))),
    "zipf": (20000, _zipf_counts(20000, 200, 0.7, 2)),
    "one_hot_item": (5010, [5000, 10]),
    "two_equal": (2000, [1000, 1000]),
    "no_slots": (7, [0, 0]),
    "no_ids": (7, []),
    "no_rows": (0, [5000, 10]),
}


@pytest.mark.parametrize("name", sorted(COLUMN_COUNTS))
def test_columns(name):
    n, counts = COLUMN_COUNTS[name]
    seen = set()
    for lane in LANES:
        W = sa.window_rule("columns", n, counts, item_lane=lane)
        assert W == wr.columns(n, counts, lane), (lane, W)
        seen.add(W)
        # amd:window overrides everything
        assert sa.window_rule("columns", n, counts, item_lane=lane, window=300) == wr.columns(n, counts, lane, window=300) == max(1, -(-n // 300))
        # window_per_target out of the way (tests/test_gpu_shared_hot_window.py): the cap alone is left
        far = sa.window_rule("columns", n, counts, item_lane=lane, per_target=100000)
        assert far == wr.columns(n, counts, lane, per_target=100000), lane
        if lane[0] and n > 0:
            assert far == max(1, -(-max(list(counts) + [0]) // lane[1]))
    if name in ("uniform", "zipf", "one_hot_item"):
        assert len(seen) >= 3, seen     # the cases move the count: the default term, the cap, the mean over entries


def test_columns_search_brackets_the_hand_computed_cases():
    """tests/test_pair_hot_checker.py's literals, through the engine"""
    assert sa.window_rule("columns", 5010, [5000, 10], item_lane=(30, 2048)) == 208
    assert sa.window_rule("columns", 5010, [5000, 10], item_lane=(5, 100)) == 50
    assert sa.window_rule("columns", 2000, [1000, 1000], item_lane=(128, 2048)) == 42
    assert sa.window_rule("columns", 5010, [5000, 10]) == 208


def _csr_case(shared, tables):
    """20 000 rows: 200 Zipf items, 8 global ids, four dense shared buckets of 5 000 (or no shared rows); with tables, the first 20 items and
    the last bucket are side-table children"""
    n = 20000
    ci, cg = _zipf_counts(n, 200, 0.7, 3), np.full(8, n // 8)
    cs = np.full(4, 5000) if shared else np.zeros(0, np.int64)
    ichild = uchild = None
    if tables:
        ichild = (np.arange(200) < 20).astype(np.uint8)
        uchild = np.array([0, 0, 0, 1], np.uint8) if shared else np.zeros(0, np.uint8)
    return n, ci, cg, cs, ichild, uchild


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("tables", [True, False])
def test_csr(shared, tables):
    n, ci, cg, cs, ichild, uchild = _csr_case(shared, tables)
    seen = set()
    for shared_lane in ((0, 0), (12, 512), (3, 64)):
        for item_lane in ((0, 0), (8, 2048), (24, 128)):
            for knobs in ({}, {"per_target": 100000}, {"per_target_child": 12, "per_target_shared": 24}, {"window": 777}):
                W = sa.window_rule("csr", n, ci, cg, cs, ichild, uchild, shared_lane=shared_lane, item_lane=item_lane, **knobs)
                assert W == wr.csr(n, ci, cg, cs, ichild, uchild, shared_lane, item_lane, **knobs), (shared_lane, item_lane, knobs, W)
                seen.add(W)
    assert len(seen) >= 3, seen     # the lanes and the knobs move the count
    if shared and not tables:   # the default the GPU tests name: dense buckets at window_per_target_shared = 12 updates per window
        assert sa.window_rule("csr", n, ci, cg, cs) == -(-5000 // 12)


def test_csr_without_rows():
    assert sa.window_rule("csr", 0, [3, 4], [7], [7]) == wr.csr(0, [3, 4], [7], [7]) == 1


@pytest.mark.parametrize("fb_scale", [0.01, 4000.0])   # the feedback mass far below every other term, and binding
def test_blocks(fb_scale):
    n, nb = 12000, 3000
    ci, cs = _zipf_counts(n, 200, 0.7, 4), np.full(4, n // 4)
    mass = np.random.default_rng(5).uniform(0.5, 1.5, 2000) * fb_scale
    seen = set()
    for shared_lane in ((0, 0), (12, 512), (8, 64)):
        for item_lane in ((0, 0), (12, 512), (64, 128)):
            for num_block in (nb, 5):      # (5: fewer blocks than the rule's windows)
                for knobs in ({}, {"window": 4000}, {"per_target_fb": 4}):
                    W = sa.window_rule("blocks", n, ci, (), cs, fb_mass=mass, num_block=num_block, shared_lane=shared_lane, item_lane=item_lane, **knobs)
                    want = wr.blocks(n, num_block, ci, (), cs, mass, shared_lane, item_lane, **knobs)
                    assert W == want, (shared_lane, item_lane, num_block, knobs, W, want)
                    assert W <= num_block
                    seen.add(W)
    assert 5 in seen and len(seen) >= 4, seen
    fb = wr.windows(n, [0.0, 0.0, float(np.dot(mass, mass) / mass.sum())])   # the feedback term alone
    assert (sa.window_rule("blocks", n, ci, (), cs, fb_mass=mass, num_block=nb) == fb) == (fb_scale > 1), fb


@pytest.fixture(scope="module")
def orders():
    return {order: woc.triples_with_holdout(N, NU, NI, SEED, order)[0][1] for order in woc.ORDERS}


@pytest.mark.parametrize("order", woc.ORDERS)
@pytest.mark.parametrize("sub", [0, HOT_SUB])
def test_as_cut(orders, order, sub):
    """the four file orders at the sizes of tests/test_window_orders.py, both lanes"""
    item = orders[order]
    cap = HOT_MAX if sub else PER_MAX
    W = sa.window_rule_as_cut(PARENT_W, [item], NI, PER, cap, sub)
    assert W == wr.as_cut(PARENT_W, [item], NI, sub, cap), (order, sub, W)
    assert (W == PARENT_W) == (order in ("shuffled", "user"))
    # two columns of one class (rank pairs), and a search that runs out of rounds
    both = sa.window_rule_as_cut(PARENT_W, [item, item[::-1].copy()], NI, PER, cap, sub)
    assert both == wr.as_cut(PARENT_W, [item, item[::-1]], NI, sub, cap)
    assert sa.window_rule_as_cut(PARENT_W, [item], NI, PER, cap, sub, rounds=1) == wr.as_cut(PARENT_W, [item], NI, sub, cap, rounds=1)


S, M, E, D = 1, 3, 2, 0   # svdpp_tag: START, MIDDLE, END, DEFAULT


@pytest.mark.parametrize("tags", [
    [D] * 12,
    [D, S, M, E, D, D, S, E, D, D, D, D],          # spans that straddle the even positions of W = 2, 3, 4, 6
    [D, S, M, M, M, M, M, M, M, E, D, D],          # one span over several cut positions
    [S, M, M, M, M, M, M, M, M, M, M, E],          # one span over all of them
    [S, E] * 6,
    [],
], ids=["default", "straddle", "long_span", "one_span", "pairs", "empty"])
def test_block_cuts(tags):
    for W in sorted({1, 2, 3, 4, 6, max(len(tags), 1)}):
        cut = sa.window_block_cuts(tags, W).tolist()
        assert cut == wr.block_cuts(tags, W), (W, cut)
        assert cut[0] == 0 and cut[-1] == len(tags) and len(cut) == W + 1 and cut == sorted(cut)
        for pos in cut[1:-1]:
            assert pos in (0, len(tags)) or tags[pos - 1] in (E, D), (W, cut)     # no cut inside a START .. END span

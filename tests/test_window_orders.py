"""The window rule on clustered file orders, on the CPU checkers alone (tests/window_order_cases.py; svdf_wseq_rule.h: wseq_actual_columns; DESIGN.md
section 6r).  The per-pass rule takes a row's c updates as spread evenly over the W windows and cuts the file at equal positions; on a file sorted
by item, or one that arrives in bursts, one window holds all of an item's ratings.  This test keeps the inputs of tests/test_gpu_window_orders.py
honest: at the parent's window count the item and burst orders break the accuracy contract by at least 5x (so they bite), and at the count of the
rule evaluated on the windows as cut every order keeps it.  The Python version of that rule is tests/window_rule.py.

Checkers: OracleTrainer.update_batch_stale plus the window's add (the window step without a lane), update_window_substeps (ordered sub-steps of
window_hot_sub = 128); dRMSE on the held-out tenth against update_batch (the exact sequential pass) on the same file order.

Measured (profiles/r17_window_orders.md): slack 1.5, seeds 21-23: |dRMSE| <= 5.1e-5 on the item and burst orders, both lanes."""
import numpy as np
import pytest

import cases
import window_order_cases as woc
import window_rule as wr
from svdfeature_amd import CSRData

NU, NI, N, K, PASSES, SEED = 20000, 500, 200000, 16, 3, 22
PER, PER_MAX, HOT_SUB, HOT_MAX = 24, 128, 128, 2048   # window_per_target, window_per_target_max, window_hot_sub, window_hot_max (include/svdfeature_amd.h)
SLACK = wr.SLACK                                     # svdf_wseq_rule.h: kWseqSlack
PARENT_W = 17                                        # the per-pass rule on these inputs, either lane, any order (tests/test_gpu_window_orders.py pins it on the engine with window_count_actual = 0)
CONTRACT = 1e-4


def _oracle():
    from oracle import oracle
    oracle.build()
    o = oracle.OracleTrainer("port", 0, 0)
    o.seed(10)
    for k, v in cases.conf_with(cases.BASICMF_CONF, num_user=NU, num_item=NI, num_factor=K):
        o.set_param(k, v)
    o.init_model()
    o.init_trainer()
    return o


def heldout_rmse(train, held, W, sub):
    """W = None: the exact pass; else W windows at equal positions through the checker (sub = 0: stale sums, else ordered sub-steps of sub)"""
    u, i, r = train
    o = _oracle()
    n = len(r)
    ws = [CSRData.from_triples(u, i, r)] if W is None else [CSRData.from_triples(u[a:b], i[a:b], r[a:b]) for a, b in woc.window_cuts(n, W)]
    for _ in range(PASSES):
        for d in ws:
            if W is None:
                o.update_batch(d)
            elif sub > 0:
                o.update_window_substeps(d, sub)
            else:
                dW, db, _ = o.update_batch_stale(d)
                o.set_view("W_item", o.view("W_item") + dW)
                o.set_view("i_bias", o.view("i_bias") + db)
    p = o.predict_batch(CSRData.from_triples(*held))
    return cases.rmse(p, held[2]) if np.isfinite(p).all() else float("nan")


@pytest.fixture(scope="module")
def inputs():
    """order -> (train in that order, held out, the exact pass's held-out RMSE on that order)"""
    out = {}
    for order in woc.ORDERS:
        train, held = woc.triples_with_holdout(N, NU, NI, SEED, order)
        out[order] = (train, held, heldout_rmse(train, held, None, 0))
    return out


def test_the_per_pass_rule_gives_the_parents_count_on_every_order(inputs):
    for order in woc.ORDERS:
        counts = np.bincount(inputs[order][0][1].astype(np.int64), minlength=NI)
        assert wr.columns(N, counts) == PARENT_W and wr.columns(N, counts, (HOT_SUB, HOT_MAX)) == PARENT_W, order


@pytest.mark.parametrize("order", ["item", "burst"])
def test_the_parents_cut_breaks_the_contract_on_clustered_orders(inputs, order):
    train, held, exact = inputs[order]
    worst, per_entry = woc.window_counts(train[1], NI, PARENT_W)
    print(order, "W", PARENT_W, "worst", worst, "mean", woc.mean_met(per_entry, 0))
    assert worst > PER_MAX                                   # "at most window_per_target_max" does not hold on the windows as cut
    assert woc.mean_met(per_entry, 0) > 5 * PER
    d = heldout_rmse(train, held, PARENT_W, 0) - exact
    print(order, "dRMSE at the parent's cut, lane off", d)
    assert not abs(d) <= 5 * CONTRACT, d                     # (NaN counts as broken)


@pytest.mark.parametrize("order", woc.ORDERS)
@pytest.mark.parametrize("sub", [0, HOT_SUB])
def test_the_rule_on_the_windows_as_cut_keeps_the_contract(inputs, order, sub):
    train, held, exact = inputs[order]
    cap = HOT_MAX if sub else PER_MAX
    W = wr.as_cut(PARENT_W, [train[1]], NI, sub, cap)
    worst, per_entry = woc.window_counts(train[1], NI, W)
    assert worst <= cap * SLACK and woc.mean_met(per_entry, sub) <= PER * SLACK
    if order in ("shuffled", "user"):
        assert W == PARENT_W, (order, W)                     # the control: files in random item order keep the parent's windows
    else:
        assert W > 10 * PARENT_W, (order, W)
    d = heldout_rmse(train, held, W, sub) - exact
    print(order, "sub", sub, "W", W, "worst", worst, "dRMSE", d)
    assert abs(d) <= CONTRACT, (order, sub, W, d)
    if order in ("item", "burst"):
        assert abs(d) <= 7e-5, (order, sub, W, d)            # the room tests/test_gpu_window_orders.py needs (its kernels equal these checkers bit for bit)

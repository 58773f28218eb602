#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the ordered sub-steps for hot item rows of user-group (SVD++) blocks (knob
`window_block_item_sub` on a format_type 1 trainer; svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_walk<LPI, true, true>,
k_wunit_apply_hot<LPI, true, true>): random widths, links, regularisers (per-id item decay ranges, nonnegative users, no
user bias, scale_lr_ufeedback), block shapes (1 ... 12 rows, START / MIDDLE / END spans, feedback lists of 0 ... 90 ids, one or two item entries
per row, non-unit item values, 2 ... 14 items), with and without shared user ids (`amd:shared_user_from`, then `window_block_sub` on at random as
well), sub-steps of 1 ... 40, window counts, passes and the knobs wunit_fast / wunit_defer_fb -- `amd:step = minibatch` on one GPU against the
checker of tests/window_sim.py, bit for bit, and counters 35 / 36 against the checker's counts of hot rows.
usage: python tests/fuzz_block_item_hot.py --iters 150 --seed 1"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import svdfeature_amd as sa
import window_sim as ws
from svdfeature_amd import BlockArrays, CSRData, PlusBlock


def redraw_items(rng, blocks, ni, two, vals):
    out = []
    for b in blocks:
        rows = []
        for r in range(b.data.num_row):
            label, ng, nu, _, idx, val = b.data.row(r)
            v = lambda: float(rng.choice([1.0, 0.5, 2.0, 0.25])) if vals else 1.0   # noqa: E731
            i = int(idx[ng + nu])
            it = [(i, v())]
            if two and ni > 1 and rng.random() < 0.7:
                it.append(((i + 1 + int(rng.integers(0, ni - 1))) % ni, v()))
                it = it[::-1] if rng.random() < 0.5 else it
            rows.append((float(label), [], [(int(x), float(y)) for x, y in zip(idx[ng:ng + nu], val[ng:ng + nu])], it))
        out.append(PlusBlock(b.index_ufeedback, b.value_ufeedback, CSRData.from_rows(rows), b.extend_tag))
    return out


def one(rng):
    k = int(rng.choice([1, 3, 5, 8, 16, 33, 64, 64, 64, 100, 128, 128, 200, 256]))
    npv, ns, ni, nf = int(rng.integers(3, 60)), int(rng.integers(1, 8)), int(rng.integers(2, 15)), int(rng.integers(1, 100))
    active = int(rng.choice([0, 0, 2, 3]))
    reg = int(rng.integers(0, 4))
    extra = {}
    if rng.random() < 0.3: extra["no_user_bias"] = "1"
    if rng.random() < 0.2: extra["user_nonnegative"] = "1"
    if rng.random() < 0.3: extra["wd_item_bias"] = "0.01"
    if rng.random() < 0.4: extra["scale_lr_ufeedback"] = str(float(rng.choice([0.5, 2.0])))
    if rng.random() < 0.3: extra["wd_ufeedback_bias"] = "0.01"
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=npv + ns, num_item=ni, num_factor=k, num_ufeedback=nf, reg_method=reg, active_type=active,
                           learning_rate=str(float(rng.choice([0.005, 0.01, 0.02]))), wd_ufeedback="0.004", ufeedback_init_sigma="0.01", **extra)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    if rng.random() < 0.3 and ni >= 2:
        cut = int(rng.integers(1, ni))
        conf += [("ip:wd", "0.01"), ("ip:bound", str(cut)), ("ip:wd", "0.002"), ("ip:bound", str(ni))]
    shared = bool(rng.random() < 0.4)
    max_shared = min(ns, int(rng.integers(1, 5))) if shared else 0
    nblocks = int(rng.integers(1, 40))
    blocks = ws.shared_blocks(rng, nblocks, npv, ns, ni, nf, max_rows=int(rng.integers(1, 13)), max_fb=min(nf, int(rng.choice([0, 3, 20, 90]))),
                               max_shared=max_shared, min_shared=0, per_row=bool(rng.random() < 0.4), uvals=bool(rng.random() < 0.5) if shared else False,
                               split_every=int(rng.choice([0, 2, 4])), binary=active != 0)
    two, vals = bool(rng.random() < 0.4), bool(rng.random() < 0.5)
    blocks = redraw_items(rng, blocks, ni, two, vals)
    ba = BlockArrays.from_blocks(blocks)
    window = int(rng.integers(max(1, ba.num_row // 4), ba.num_row + 1))
    passes = int(rng.integers(1, 3))
    isub = int(rng.choice([1, 2, 3, 5, 8, 12, 40]))
    if reg == 2:
        isub = 1   # the projection overshoots when several changes of a row are formed against one value: NaN, whose bits need not agree
    sub = int(rng.choice([0, 1, 3, 8])) if shared else 0
    knobs = {"wunit_fast": int(rng.choice([0, 2, 3])), "wunit_defer_fb": int(rng.integers(0, 2)), "window_block_item_sub": isub}
    if sub:
        knobs["window_block_sub"] = sub
    t = sa.Trainer(1, active)
    t.seed(10)
    for kk, v in conf + [("amd:step", "minibatch"), ("amd:window", str(window))] + ([("amd:shared_user_from", str(npv))] if shared else []):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    for kk, v in knobs.items():
        t.set_knob(kk, v)
    ds = t.dataset_from_blocks(ba)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.make_oracle(conf, active=active, user_group=True)
    nuh, nih = ws.simulate_blocks(o, ba, npv if shared else npv + ns, ds.num_batches, passes, isub=isub, sub=sub, user_bias=extra.get("no_user_bias") != "1")
    bad = []
    for name in ws.VIEWS:
        a, b = t.view(name), o.view(name)
        if a is None or b is None or b.size == 0:
            continue
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append(name)
        elif not np.isfinite(b).all():
            bad.append(name + ": not finite")
    if t.counter(36) != nih:
        bad.append("counter 36: %d, the checker's hot item rows: %d" % (t.counter(36), nih))
    if t.counter(35) != nuh:
        bad.append("counter 35: %d, the checker's hot user rows: %d" % (t.counter(35), nuh))
    desc = dict(k=k, np=npv, ns=ns, ni=ni, nf=nf, blocks=nblocks, rows=ba.num_row, active=active, reg=reg, extra=extra, shared=shared, two=two, vals=vals,
                windows=ds.num_batches, passes=passes, knobs=knobs, hot_items=nih, hot_users=nuh)
    ds.close(); t.close(); o.close()
    return bad, desc


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails, hot, with_hot = 0, 0, 0
    for it in range(iters):
        bad, desc = one(rng)
        hot += desc["hot_items"]; with_hot += desc["hot_items"] > 0
        if bad:
            fails += 1
            print(json.dumps({"iter": it, "mismatch": bad, **desc}), flush=True)
        elif verbose and it % 50 == 0:
            print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "block_item_hot", "iters": iters, "seed": seed, "mismatches": fails, "hot_item_rows_applied": hot, "configurations_with_hot_items": with_hot}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

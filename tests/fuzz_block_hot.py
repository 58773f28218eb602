#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the ordered sub-steps for hot shared user rows of user-group (SVD++) blocks
(knob `window_block_sub` under `amd:shared_user_from` on a format_type 1 trainer; svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_walk<LPI, true, true>,
k_wunit_apply_hot<LPI, false, true>): random widths, links, regularisers (per-id user decay ranges over the shared ids,
nonnegative users, no user bias, scale_lr_ufeedback), block shapes (1 ... 12 rows, START / MIDDLE / END spans, feedback lists of 0 ... 90 ids,
0 ... 5 shared ids with the private entry anywhere, one section per block or per row, non-unit values), sub-steps of 1 ... 40, window counts,
passes and the knobs wunit_fast / wunit_defer_fb -- `amd:step = minibatch` on one GPU against the checker of tests/window_sim.py, bit for bit,
and counter 35 against the checker's count of hot rows.
usage: python tests/fuzz_block_hot.py --iters 150 --seed 1"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import svdfeature_amd as sa
import window_sim as ws
from svdfeature_amd import BlockArrays


def one(rng):
    k = int(rng.choice([1, 3, 8, 16, 33, 64, 64, 64, 100, 128, 128, 192, 256]))
    npv, ns, ni, nf = int(rng.integers(3, 60)), int(rng.integers(1, 8)), int(rng.integers(2, 50)), int(rng.integers(1, 100))
    active = int(rng.choice([0, 0, 2, 3]))
    reg = int(rng.integers(0, 4))
    extra = {}
    if rng.random() < 0.3: extra["no_user_bias"] = "1"
    if rng.random() < 0.2: extra["user_nonnegative"] = "1"
    if rng.random() < 0.3: extra["wd_user_bias"] = "0.01"
    if rng.random() < 0.4: extra["scale_lr_ufeedback"] = str(float(rng.choice([0.5, 2.0])))
    if rng.random() < 0.3: extra["wd_ufeedback_bias"] = "0.01"
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=npv + ns, num_item=ni, num_factor=k, num_ufeedback=nf, reg_method=reg, active_type=active,
                           learning_rate=str(float(rng.choice([0.005, 0.01, 0.02]))), wd_ufeedback="0.004", ufeedback_init_sigma="0.01", **extra)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    if rng.random() < 0.3:
        cut = int(rng.integers(1, npv + ns))
        conf += [("up:wd", "0.01"), ("up:bound", str(cut)), ("up:wd", "0.002"), ("up:bound", str(npv + ns))]
    per_row = bool(rng.random() < 0.4)
    uvals = rng.choice(["", "shared", "all"], p=[0.3, 0.5, 0.2])
    max_shared = min(ns, int(rng.integers(1, 6)))
    nblocks = int(rng.integers(1, 40))
    blocks = ws.shared_blocks(rng, nblocks, npv, ns, ni, nf, max_rows=int(rng.integers(1, 13)), max_fb=min(nf, int(rng.choice([0, 3, 20, 90]))),
                               max_shared=max_shared, min_shared=int(rng.integers(0, max_shared + 1)), per_row=per_row,
                               uvals={"": False, "shared": True, "all": "all"}[str(uvals)], split_every=int(rng.choice([0, 2, 4])), binary=active != 0)
    ba = BlockArrays.from_blocks(blocks)
    window = int(rng.integers(max(1, ba.num_row // 4), ba.num_row + 1))
    passes = int(rng.integers(1, 3))
    sub = int(rng.choice([1, 2, 3, 5, 8, 12, 40]))
    knobs = {"wunit_fast": int(rng.choice([0, 2, 3])), "wunit_defer_fb": int(rng.integers(0, 2)), "window_block_sub": sub}
    t = sa.Trainer(1, active)
    t.seed(10)
    for kk, v in conf + [("amd:step", "minibatch"), ("amd:window", str(window)), ("amd:shared_user_from", str(npv))]:
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
    nhot, _ = ws.simulate_blocks(o, ba, npv, ds.num_batches, passes, sub=sub, user_bias=extra.get("no_user_bias") != "1")
    bad = []
    for name in ws.VIEWS:
        a, b = t.view(name), o.view(name)
        if a is None or b is None or b.size == 0:
            continue
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            bad.append(name)
    if t.counter(35) != nhot:
        bad.append("counter 35: %d, the checker's hot rows: %d" % (t.counter(35), nhot))
    desc = dict(k=k, np=npv, ns=ns, ni=ni, nf=nf, blocks=nblocks, rows=ba.num_row, active=active, reg=reg, extra=extra, per_row=per_row, uvals=str(uvals),
                max_shared=max_shared, windows=ds.num_batches, passes=passes, knobs=knobs, hot=nhot, general=t.counter(34))
    ds.close(); t.close(); o.close()
    return bad, desc


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails, hot, with_hot = 0, 0, 0
    for it in range(iters):
        bad, desc = one(rng)
        hot += desc["hot"]; with_hot += desc["hot"] > 0
        if bad:
            fails += 1
            print(json.dumps({"iter": it, "mismatch": bad, **desc}), flush=True)
        elif verbose and it % 50 == 0:
            print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "block_hot", "iters": iters, "seed": seed, "mismatches": fails, "hot_rows_applied": hot, "configurations_with_hot_rows": with_hot}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

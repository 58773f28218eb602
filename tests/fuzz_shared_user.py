#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the window step with shared user rows (`amd:shared_user_from`, svdf_wunit.cpp,
svdf_k_wunit.hip): random widths, links, regularisers (per-id user decay ranges over the shared ids, nonnegative users, no user bias), row
shapes (0 ... 4 global entries, 0 ... 4 shared ids with the private entry anywhere, non-unit values, one or two item entries), hot and rare
shared ids, window sizes and passes -- `amd:step = minibatch` on one GPU against the checker of tests/window_sim.py, bit for bit.
usage: python tests/fuzz_shared_user.py --iters 300 --seed 1"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import svdfeature_amd as sa
import window_sim as ws
from svdfeature_amd import CSRData

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def one(rng):
    k = int(rng.choice([1, 3, 8, 16, 33, 64, 64, 100, 128, 128, 200, 256]))
    npv, ns, ni, ng = int(rng.integers(5, 80)), int(rng.integers(1, 120)), int(rng.integers(2, 50)), int(rng.choice([0, 0, 5, 20]))
    n = int(rng.integers(20, 400))
    active = int(rng.choice([0, 0, 2, 3]))
    reg = int(rng.integers(0, 4))
    extra = {}
    if rng.random() < 0.3: extra["no_user_bias"] = "1"
    if rng.random() < 0.3: extra["user_nonnegative"] = "1"
    if rng.random() < 0.3: extra["wd_user_bias"] = "0.01"
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=npv + ns, num_item=ni, num_global=ng, num_factor=k, reg_method=reg, active_type=active,
                           wd_global="0.002", learning_rate=str(float(rng.choice([0.005, 0.01, 0.02]))), **extra)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    if rng.random() < 0.3:
        cut = int(rng.integers(1, npv + ns))
        conf += [("up:wd", "0.01"), ("up:bound", str(cut)), ("up:wd", "0.002"), ("up:bound", str(npv + ns))]
    hot = tuple(npv + int(x) for x in rng.choice(ns, size=min(ns, int(rng.integers(0, 3))), replace=False))
    d = ws.shared_rows(rng, n, npv, ns, ni, num_global=ng, max_g=int(rng.integers(0, 5)) if ng else 0,
                                    max_shared=min(ns, int(rng.integers(0, 5))), uvals=rng.random() < 0.6, hot=hot, hot_p=float(rng.uniform(0, 1)))
    if rng.random() < 0.3:   # a second item entry in some rows
        rows = []
        for r in range(d.num_row):
            label, g_, nu_, ni_, idx, val = d.row(r)
            gl = [(int(idx[j]), float(val[j])) for j in range(g_)]
            us = [(int(idx[j]), float(val[j])) for j in range(g_, g_ + nu_)]
            it = [(int(idx[g_ + nu_]), 1.0)]
            x = int(rng.integers(0, ni))
            if rng.random() < 0.4 and x != it[0][0]:
                it.append((x, -0.5))
            rows.append((label, gl, us, it))
        d = CSRData.from_rows(rows)
    if active != 0:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    window = int(rng.integers(1, n + 1))
    passes = int(rng.integers(1, 4))
    t = sa.Trainer(0, active)
    t.seed(10)
    for kk, v in conf + [("amd:step", "minibatch"), ("amd:window", str(window)), ("amd:shared_user_from", str(npv))]:
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    ds = t.dataset_from_csr(d)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, npv, ds.num_batches, passes,
                                 user_bias=extra.get("no_user_bias") != "1")
    bad = [name for name in VIEWS if not np.array_equal(t.view(name).view(np.uint32), o.view(name).view(np.uint32))]
    desc = dict(k=k, np=npv, ns=ns, ni=ni, ng=ng, n=n, active=active, reg=reg, extra=extra, hot=hot, windows=ds.num_batches, passes=passes)
    ds.close(); t.close(); o.close()
    return bad, desc


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails = 0
    for it in range(iters):
        bad, desc = one(rng)
        if bad:
            fails += 1
            print(json.dumps({"iter": it, "mismatch": bad, **{k: (v if not isinstance(v, tuple) else list(v)) for k, v in desc.items()}}), flush=True)
        elif verbose and it % 50 == 0:
            print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "shared_user", "iters": iters, "seed": seed, "mismatches": fails}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

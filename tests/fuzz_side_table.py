#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the window step with feature_user / feature_item side tables (svdf_wunit.cpp,
svdf_k_wunit.hip): random widths, links, regularisers (per-id decay ranges on both sides, nonnegative users, no user
bias, bias decays), tables (user only, item only, both; 0 ... 3 children per id, hot and rare children, ids without a table row), row shapes
(0 ... 3 global entries, 0 ... 3 shared user ids with the private entry anywhere, 1 ... 3 items, values other than 1), window sizes and
passes -- `amd:step = minibatch` on one GPU against the checker of tests/window_sim.py, bit for bit.  Rows that reach one target twice
(which the step refuses) are dropped from the draw.
usage: python tests/fuzz_side_table.py --iters 150 --seed 1"""
import argparse, json, os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import svdfeature_amd as sa
import window_sim as ws

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias")


def same(a, b):
    """bit for bit, except that a value both sides lost to NaN (a draw whose training diverges) matches whatever its payload"""
    nan = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(nan, 0, a.view(np.uint32)), np.where(nan, 0, b.view(np.uint32)))


def one(rng, tmp):
    k = int(rng.choice([1, 3, 8, 16, 33, 64, 64, 100, 128, 128, 200, 256]))
    npv, ns = int(rng.integers(5, 60)), int(rng.integers(1, 80))
    nt, na, ng = int(rng.integers(2, 40)), int(rng.integers(1, 40)), int(rng.choice([0, 0, 5, 20]))
    ni = nt + na
    n = int(rng.integers(20, 300))
    active = int(rng.choice([0, 0, 2, 3]))
    reg = int(rng.integers(0, 4))
    which = str(rng.choice(["user", "item", "both", "both"]))
    key = which != "item" or rng.random() < 0.5
    extra = {}
    if rng.random() < 0.3: extra["no_user_bias"] = "1"
    if rng.random() < 0.3: extra["user_nonnegative"] = "1"
    if rng.random() < 0.3: extra["wd_user_bias"] = "0.01"
    if rng.random() < 0.3: extra["wd_item_bias"] = "0.02"
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=npv + ns, num_item=ni, num_global=ng, num_factor=k, reg_method=reg, active_type=active,
                           wd_global="0.002", learning_rate=str(float(rng.choice([0.005, 0.01, 0.02]))), **extra)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    if rng.random() < 0.3:
        cut = int(rng.integers(1, npv + ns))
        conf += [("up:wd", "0.01"), ("up:bound", str(cut)), ("up:wd", "0.002"), ("up:bound", str(npv + ns))]
    if rng.random() < 0.3:
        cut = int(rng.integers(1, ni))
        conf += [("ip:wd", "0.003"), ("ip:bound", str(cut)), ("ip:wd", "0.015"), ("ip:bound", str(ni))]
    tu, ti = [], []
    if which != "item":
        hot = tuple(npv + int(x) for x in rng.choice(ns, size=min(ns, int(rng.integers(0, 3))), replace=False))
        tu = ws.random_table(rng, int(rng.integers(1, npv + ns + 1)), npv, npv + ns, int(rng.integers(1, 4)), p_none=float(rng.uniform(0, 0.6)),
                              hot=hot, hot_p=float(rng.uniform(0, 1)))
        conf += [("feature_user", ws.write_table(os.path.join(tmp, "fu.txt"), tu))]
    if which != "user":
        lo = 0 if rng.random() < 0.3 else nt   # children among the tracks themselves, or among the attribute ids after them
        hot = tuple(lo + int(x) for x in rng.choice(ni - lo, size=min(ni - lo, int(rng.integers(0, 3))), replace=False))
        ti = ws.random_table(rng, int(rng.integers(1, nt + 1)), lo, ni, int(rng.integers(1, 4)), p_none=float(rng.uniform(0, 0.6)),
                              hot=hot, hot_p=float(rng.uniform(0, 1)))
        conf += [("feature_item", ws.write_table(os.path.join(tmp, "fi.txt"), ti))]
    tu, ti = [ws.read_table(dict(conf)[x]) if x in dict(conf) else [] for x in ("feature_user", "feature_item")]
    B = npv if key else npv + ns
    d = ws.table_rows(rng, n, npv, ns, nt, num_global=ng, max_g=int(rng.integers(0, 4)) if ng else 0, max_shared=int(rng.integers(0, 4)) if key else 0,
                       max_items=int(rng.integers(1, 4)), uvals=rng.random() < 0.6, ivals=rng.random() < 0.7)
    d = ws.drop_rows_reaching_twice(d, B, tu, ti)
    if active != 0:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    window = int(rng.integers(1, max(d.num_row, 1) + 1))
    passes = int(rng.integers(1, 4))
    return dict(k=k, npv=npv, ns=ns, nt=nt, na=na, ng=ng, active=active, reg=reg, which=which, key=key, extra=extra, conf=conf, tu=tu, ti=ti,
                B=B, d=d, window=window, passes=passes)


def check(c, knobs=()):
    k, npv, ns, nt, na, ng, active, reg, which, key, extra, conf, tu, ti, B, d, window, passes = (
        c[x] for x in ("k", "npv", "ns", "nt", "na", "ng", "active", "reg", "which", "key", "extra", "conf", "tu", "ti", "B", "d", "window", "passes"))
    t = sa.Trainer(0, active)
    t.seed(10)
    for kk, v in conf + [("amd:step", "minibatch"), ("amd:window", str(window))] + ([("amd:shared_user_from", str(npv))] if key else []):
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    for kk, v in knobs:
        t.set_knob(kk, v)
    ds = t.dataset_from_csr(d)
    for _ in range(passes):
        t.train_dataset(ds)
    t.synchronize()
    o = ws.simulate_rows(ws.make_oracle(conf, active=active), d, B, ds.num_batches, passes, fu=tu, fi=ti,
                     user_bias=extra.get("no_user_bias") != "1")
    bad = [name for name in VIEWS if not same(t.view(name), o.view(name))]
    desc = dict(k=k, np=npv, ns=ns, nt=nt, na=na, ng=ng, n=d.num_row, active=active, reg=reg, tables=which, key=key, extra=extra,
                windows=ds.num_batches, passes=passes, diverged=bool(any(np.isnan(o.view(name)).any() for name in VIEWS)))
    views = {name: (t.view(name).copy(), o.view(name).copy()) for name in VIEWS}
    ds.close(); t.close(); o.close()
    return bad, desc, views


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails = diverged = 0
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(iters):
            bad, desc, _ = check(one(rng, tmp))
            diverged += desc["diverged"]
            if bad:
                fails += 1
                print(json.dumps({"iter": it, "mismatch": bad, **desc}), flush=True)
            elif verbose and it % 25 == 0:
                print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "side_table", "iters": iters, "seed": seed, "mismatches": fails, "diverged": diverged}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

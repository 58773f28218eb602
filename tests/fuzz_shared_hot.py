#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the ordered sub-steps for hot shared user rows in the window step (knob
`window_shared_sub`; svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_apply_shared).  The draws are those of
tests/fuzz_side_table.py -- random widths, links, regularisers (per-id decay ranges, nonnegative users, no user bias, bias decays), tables
(none, user only, both; hot and rare children), row shapes (0 ... 3 global entries, 0 ... 3 shared user ids with the private entry anywhere,
1 ... 3 items, values other than 1), window sizes and passes -- with amd:shared_user_from always set, few shared ids in half of the draws (so
that a data row holds several hot entries) and a random sub-step size 1 ... 16: `amd:step = minibatch` on one GPU against the checker of
tests/window_sim.py, bit for bit.
usage: python tests/fuzz_shared_hot.py --iters 150 --seed 1"""
import argparse, json, os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import fuzz_side_table
import svdfeature_amd as sa
import window_sim as ws

VIEWS = fuzz_side_table.VIEWS
same = fuzz_side_table.same


def one(rng, tmp):
    k = int(rng.choice([1, 3, 8, 16, 33, 64, 64, 100, 128, 128, 200, 256]))
    npv = int(rng.integers(5, 60))
    ns = int(rng.integers(1, 6)) if rng.random() < 0.5 else int(rng.integers(6, 80))
    nt, na, ng = int(rng.integers(2, 40)), int(rng.integers(1, 40)), int(rng.choice([0, 0, 5, 20]))
    ni = nt + na
    n = int(rng.integers(20, 300))
    active = int(rng.choice([0, 0, 2, 3]))
    reg = int(rng.integers(0, 4))
    which = str(rng.choice(["none", "none", "user", "both"]))
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
    tu, ti = [], []
    if which != "none":
        hot = tuple(npv + int(x) for x in rng.choice(ns, size=min(ns, int(rng.integers(0, 3))), replace=False))
        tu = ws.random_table(rng, int(rng.integers(1, npv + ns + 1)), npv, npv + ns, int(rng.integers(1, 4)), p_none=float(rng.uniform(0, 0.6)),
                              hot=hot, hot_p=float(rng.uniform(0, 1)))
        conf += [("feature_user", ws.write_table(os.path.join(tmp, "fu.txt"), tu))]
    if which == "both":
        hot = tuple(nt + int(x) for x in rng.choice(na, size=min(na, int(rng.integers(0, 3))), replace=False))
        ti = ws.random_table(rng, int(rng.integers(1, nt + 1)), nt, ni, int(rng.integers(1, 4)), p_none=float(rng.uniform(0, 0.6)),
                              hot=hot, hot_p=float(rng.uniform(0, 1)))
        conf += [("feature_item", ws.write_table(os.path.join(tmp, "fi.txt"), ti))]
    tu, ti = [ws.read_table(dict(conf)[x]) if x in dict(conf) else [] for x in ("feature_user", "feature_item")]
    d = ws.table_rows(rng, n, npv, ns, nt, num_global=ng, max_g=int(rng.integers(0, 4)) if ng else 0, max_shared=int(rng.integers(1, 4)),
                       max_items=int(rng.integers(1, 4)), uvals=rng.random() < 0.6, ivals=rng.random() < 0.7)
    d = ws.drop_rows_reaching_twice(d, npv, tu, ti)
    if active != 0:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    window = int(rng.integers(1, max(d.num_row, 1) + 1))
    return dict(k=k, npv=npv, ns=ns, ng=ng, active=active, reg=reg, which=which, extra=extra, conf=conf, tu=tu, ti=ti, d=d, window=window,
                passes=int(rng.integers(1, 4)), sub=int(rng.integers(1, 17)))


def check(c):
    t = sa.Trainer(0, c["active"])
    t.seed(10)
    for kk, v in c["conf"] + [("amd:step", "minibatch"), ("amd:window", str(c["window"])), ("amd:shared_user_from", str(c["npv"]))]:
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    t.set_knob("window_shared_sub", c["sub"])
    d = c["d"]
    ds = t.dataset_from_csr(d)
    for _ in range(c["passes"]):
        t.train_dataset(ds)
    t.synchronize()
    W = ds.num_batches
    o = ws.simulate_rows(ws.make_oracle(c["conf"], active=c["active"]), d, c["npv"], W, c["passes"], sub=c["sub"], fu=c["tu"], fi=c["ti"],
                     user_bias=c["extra"].get("no_user_bias") != "1")
    bad = [name for name in VIEWS if not same(t.view(name), o.view(name))]
    hot = 0   # hot rows over the windows of one pass: how much of the draw rode the lane
    for b0, b1 in ws.row_cuts(d.num_row, W):
        cnt = {}
        for r in range(b0, b1):
            _, ng, nu, _, idx, _ = d.row(r)
            for u in ws.row_targets(idx, ng, nu, c["npv"], c["tu"], c["ti"])[0]:
                cnt[u] = cnt.get(u, 0) + 1
        hot += sum(v > c["sub"] for v in cnt.values())
    desc = dict(k=c["k"], np=c["npv"], ns=c["ns"], ng=c["ng"], n=d.num_row, active=c["active"], reg=c["reg"], tables=c["which"], extra=c["extra"],
                windows=W, passes=c["passes"], sub=c["sub"], hot_rows=hot,
                diverged=bool(any(np.isnan(o.view(name)).any() for name in VIEWS)))
    ds.close(); t.close(); o.close()
    return bad, desc


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails = diverged = with_hot = hot_rows = 0
    with tempfile.TemporaryDirectory() as tmp:
        for it in range(iters):
            bad, desc = check(one(rng, tmp))
            diverged += desc["diverged"]
            with_hot += desc["hot_rows"] > 0
            hot_rows += desc["hot_rows"]
            if bad:
                fails += 1
                print(json.dumps({"iter": it, "mismatch": bad, **desc}), flush=True)
            elif verbose and it % 25 == 0:
                print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "shared_hot", "iters": iters, "seed": seed, "mismatches": fails, "diverged": diverged,
                      "draws_with_hot_rows": with_hot, "hot_rows": hot_rows}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

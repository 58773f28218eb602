#!/usr/bin/env python3
"""SURVEY 8(d2) side-feature variant on one MI355X with the window step for shared user rows (`amd:shared_user_from`):
4 distinct global ids out of 10 K (values U(0,1)), the user id, one of 64 "age bucket" ids placed after the real users (bucket = u % 64, as in
tools/bench_variants.py) and the item; configs[1] sizes (1 M users + 64 buckets, 100 K items), k = 64.

  exact      the default exact level-scheduled pass (each bucket row is a dependency chain of n / 64 updates)
  window     amd:step = minibatch + amd:shared_user_from = 1 M, at the default rule (a shared user row meets 12 updates per window on
             average: knob window_per_target_shared) and at the window_per_target_shared values of --per-target (default 16 / 24; values above
             window_per_target_max = 128 change nothing, that cap binds on rows met as evenly as the buckets)

Throughput of the first seed (inst/s over passes 2 .. 3, fraction of 8 TB/s by algorithmic_bytes, windows per pass), then |dRMSE| of each window pass against the exact pass after
3 passes, on a held-out set, for 3 data seeds.  --n rows per pass (a prefix of the variant's 100 M: the exact pass is the slow one).
usage: python tools/sidefeat_window.py --n 2000000 --seeds 1,2,3 --out profiles/r07_sidefeat_window.md"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdfeature_amd as sa
from svdfeature_amd import CSRData

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--test", type=int, default=200_000)
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--factor", type=int, default=64)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--seeds", default="1,2,3")
ap.add_argument("--out", default="")
ap.add_argument("--per-target", default="16,24", help="window_per_target_shared values of the extra window schemes")
a = ap.parse_args()
NG, G, NB = 4, 10000, 64


def rows(rng, n):
    u = rng.integers(0, a.users, n, dtype=np.uint32)
    i = rng.integers(0, a.items, n, dtype=np.uint32)
    r = rng.integers(1, 6, n).astype(np.float32)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)   # 4 distinct ids per row
    per = NG + 3
    row_ptr = np.empty(3 * n + 1, np.int64)
    base = per * np.arange(n, dtype=np.int64)
    row_ptr[0:3 * n:3] = base; row_ptr[1:3 * n:3] = base + NG; row_ptr[2:3 * n:3] = base + NG + 2; row_ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = u; idx[:, NG + 1] = a.users + (u % NB); idx[:, NG + 2] = i
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    return CSRData(r, row_ptr.astype(np.int32), idx.ravel(), val.ravel())


def trainer(extra, knobs):
    t = sa.Trainer(0, 0)
    t.seed(10)
    conf = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("wd_global", "0.001"),
            ("num_item", a.items), ("num_user", a.users + NB), ("num_global", G), ("num_factor", a.factor)] + extra
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


WIN = [("amd:step", "minibatch"), ("amd:shared_user_from", a.users)]
SCHEMES = [("exact", [], []), ("window, default rule (shared rows 12)", WIN, [])]
SCHEMES += [("window, window_per_target_shared %d" % int(v), WIN, [("window_per_target_shared", int(v))]) for v in a.per_target.split(",") if v]

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


seeds = [int(s) for s in a.seeds.split(",")]
perf, drmse = {}, {}
for si, seed in enumerate(seeds):
    rng = np.random.default_rng(seed)
    d, test = rows(rng, a.n), rows(rng, a.test)
    rm = {}
    for name, extra, knobs in SCHEMES:
        t = trainer(extra, knobs)
        t0 = time.perf_counter()
        ds = t.dataset_from_csr(d)
        t.synchronize()
        build = time.perf_counter() - t0
        timed = []
        for p in range(a.passes):
            t0 = time.perf_counter()
            t.train_dataset(ds)
            t.synchronize()
            timed.append(time.perf_counter() - t0)
        pred = t.predict_batch(test)
        rm[name] = float(np.sqrt(np.mean((pred.astype(np.float64) - test.row_label) ** 2)))
        if si == 0:
            dt = float(np.mean(timed[1:])) if len(timed) > 1 else timed[0]
            perf[name] = dict(inst_per_s=a.n / dt, ms_per_pass=dt * 1e3, frac=ds.algorithmic_bytes / dt / 8e12, windows=ds.num_batches if ds.kind == 8 else 0,
                              kind=ds.kind, build_s=build)
        print(json.dumps({"seed": seed, "scheme": name, "rmse": rm[name], "pass_ms": [x * 1e3 for x in timed], "kind": ds.kind,
                          "batches": ds.num_batches, "build_s": build}), file=sys.stderr, flush=True)
        ds.close(); t.close()
    for name, _, _ in SCHEMES[1:]:
        drmse.setdefault(name, []).append(rm[name] - rm["exact"])

out("# Side-feature variant (SURVEY 8(d2)) with shared user rows in the window step\n")
out("%d rows per pass (a prefix of the variant's 100 M), %d users + %d bucket ids, %d items, 4 of %d globals, k = %d; %d passes; held-out %d rows; "
    "seeds %s.  tools/sidefeat_window.py\n" % (a.n, a.users, NB, a.items, G, a.factor, a.passes, a.test, a.seeds))
out("| scheme | ms / pass | inst/s | frac of 8 TB/s | windows / pass | vs exact | data set build s |")
out("|---|---|---|---|---|---|---|")
ex = perf["exact"]["inst_per_s"]
for name, _, _ in SCHEMES:
    p = perf[name]
    out("| %s | %.1f | %.3g M | %.4f | %s | %.1fx | %.1f |" % (name, p["ms_per_pass"], p["inst_per_s"] / 1e6, p["frac"], p["windows"] or "-",
                                                        p["inst_per_s"] / ex, p["build_s"]))
out("\n| scheme | dRMSE seed " + " | dRMSE seed ".join(str(s) for s in seeds) + " | max abs |")
out("|---|" + "---|" * (len(seeds) + 1))
for name, _, _ in SCHEMES[1:]:
    v = drmse[name]
    out("| %s | %s | %.2e |" % (name, " | ".join("%+.2e" % x for x in v), max(abs(x) for x in v)))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")

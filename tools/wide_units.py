#!/usr/bin/env python3
"""The window step of user units at wide factor rows (256 < num_factor <= 1024) next to the exact pass of the same build on
one MI355X -- what the parent commit can do at these widths, since it refuses the window step there.

One cell per call: --shape sidefeat (SURVEY 8(d2)'s side-feature variant as in tools/sidefeat_window.py: 4 distinct global ids of 10 K with values
U(0, 1), the user, one of 64 bucket ids after the real users through amd:shared_user_from, the item) or --shape svdpp (BASELINE configs[3]'s
implicit-feedback blocks, benchlib/synth.py: synth_user_blocks, --per-user ratings per user), and --k.

Timing (the default): two handles on the same data -- the default (exact, level-scheduled) step and `amd:step = minibatch` -- are warmed up with
one pass each and then timed ALTERNATING, --reps passes each, every pass ended by a stream synchronisation: median and min .. max of ms per pass,
inst/s, the window count and the fraction of 8 TB/s by the bytes the reference's step moves (Dataset.algorithmic_bytes).
--rmse-seeds 1,2,3: instead, per data seed, fresh handles train --passes passes each and score a held-out set: |dRMSE| of the window step
against the exact pass.  One JSON line, appended to --out.

usage: python tools/wide_units.py --shape sidefeat --k 512 --n 20000000 --out wide_units.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svdfeature_amd as sa  # noqa: E402
from benchlib import synth  # noqa: E402
from svdfeature_amd import CSRData  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["sidefeat", "svdpp"], required=True)
ap.add_argument("--k", type=int, required=True)
ap.add_argument("--n", type=int, default=20_000_000, help="rows per pass (svdpp: users x --per-user)")
ap.add_argument("--test", type=int, default=200_000)
ap.add_argument("--users", type=int, default=200_000)
ap.add_argument("--num-items", type=int, default=20_000)
ap.add_argument("--per-user", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--rmse-seeds", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
NG, G, NB = 4, 10000, 64
BASE = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("num_item", a.num_items), ("num_factor", a.k)]


def sidefeat_rows(rng, n):
    u = rng.integers(0, a.users, n, dtype=np.uint32)
    i = rng.integers(0, a.num_items, n, dtype=np.uint32)
    r = rng.integers(1, 6, n).astype(np.float32)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)   # 4 distinct ids per row
    per = NG + 3
    row_ptr = np.empty(3 * n + 1, np.int64)
    base = per * np.arange(n, dtype=np.int64)
    row_ptr[0:3 * n:3] = base; row_ptr[1:3 * n:3] = base + NG; row_ptr[2:3 * n:3] = base + NG + 2; row_ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = u; idx[:, NG + 1] = a.users + (u % NB); idx[:, NG + 2] = i
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    return CSRData(r, row_ptr.astype(np.int32), idx.ravel(), val.ravel())


def data(seed):
    """(format_type, conf, keys of the window handle, train, held-out)"""
    if a.shape == "sidefeat":
        rng = np.random.default_rng(seed)
        conf = BASE + [("wd_global", "0.001"), ("num_user", a.users + NB), ("num_global", G)]
        return 0, conf, [("amd:shared_user_from", a.users)], sidefeat_rows(rng, a.n), sidefeat_rows(rng, a.test)
    blocks = max(1, a.n // a.per_user)
    train, test = synth.synth_user_blocks(blocks, a.per_user, max(a.users, blocks), a.num_items, seed=4242 + seed)
    conf = BASE + [("num_user", max(a.users, blocks)), ("num_global", 0), ("num_ufeedback", a.num_items), ("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
    return 1, conf, [], train, test


def trainer(fmt, conf, extra):
    t = sa.Trainer(fmt, 0)
    t.seed(10)
    for key, v in conf + extra:
        t.set_param(key, str(v))
    t.init_model()
    t.init_trainer()
    return t


def build(t, fmt, d):
    return t.dataset_from_blocks(d) if fmt == 1 else t.dataset_from_csr(d)


def held_out_rmse(t, fmt, test):
    if fmt == 0:
        p = t.predict_batch(test)
        return float(np.sqrt(np.mean((p.astype(np.float64) - test.row_label) ** 2)))
    held = t.dataset_from_blocks(test)   # (a window sequence on the window handle: scored in place, bit-identical to svdf_predict_block)
    ss, cnt = t.eval_dataset(held)
    held.close()
    return float(np.sqrt(ss / cnt))


SCHEMES = (("exact", False), ("window", True))
res = {"shape": a.shape, "k": a.k, "users": a.users, "num_items": a.num_items}
if a.rmse_seeds:
    res["passes"], res["seeds"] = a.passes, []
    for seed in [int(s) for s in a.rmse_seeds.split(",")]:
        fmt, CONF, keys, train, test = data(seed)
        rm = {}
        for name, win in SCHEMES:
            t = trainer(fmt, CONF, ([("amd:step", "minibatch")] + keys) if win else [])
            ds = build(t, fmt, train)
            for _ in range(a.passes):
                t.train_dataset(ds)
            t.synchronize()
            rm[name] = held_out_rmse(t, fmt, test)
            rm[name + "_batches"] = ds.num_batches
            ds.close(); t.close()
        rm.update(seed=seed, rows=train.num_row, drmse=rm["window"] - rm["exact"])
        res["seeds"].append(rm)
        print(json.dumps(rm), file=sys.stderr, flush=True)
else:
    fmt, CONF, keys, train, _ = data(a.seed)
    n = train.num_row
    handles = {}
    for name, win in SCHEMES:
        t = trainer(fmt, CONF, ([("amd:step", "minibatch")] + keys) if win else [])
        s = time.perf_counter()
        ds = build(t, fmt, train)
        t.synchronize()
        handles[name] = {"t": t, "ds": ds, "build_s": time.perf_counter() - s, "ms": []}
        t.train_dataset(ds)   # warm-up pass
        t.synchronize()
    for _ in range(a.reps):
        for name, _ in SCHEMES:   # alternating
            h = handles[name]
            s = time.perf_counter()
            h["t"].train_dataset(h["ds"])
            h["t"].synchronize()
            h["ms"].append(1e3 * (time.perf_counter() - s))
    res.update(rows=n, reps=a.reps)
    for name, h in handles.items():
        med = float(np.median(h["ms"]))
        res[name] = {"kind": h["ds"].kind, "windows_or_levels": h["ds"].num_batches, "build_s": h["build_s"], "ms_per_pass": med, "min_ms": min(h["ms"]),
                     "max_ms": max(h["ms"]), "inst_per_s": n / med * 1e3, "frac_of_8TBps": h["ds"].algorithmic_bytes / (med * 1e-3) / 8e12,
                     "finite": bool(np.isfinite(h["t"].view("W_item")).all())}
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")

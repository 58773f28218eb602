#!/usr/bin/env python3
"""The window step at wide factor rows (256 < num_factor <= 1024) next to the exact pass of the same build on one MI355X.

One cell per call: --k, --items uniform | zipf (Zipf(0.7) over a permuted catalogue, benchlib/orders.py) or --pairs (rank pairs, sigmoid rank
loss, no user bias).  Two handles on the same data -- the default (exact, level-scheduled) step and `amd:step = minibatch` -- are warmed up with
one pass each and then timed ALTERNATING, --reps passes each, every pass ended by a stream synchronisation: median and min .. max of ms per pass,
inst/s, and for the window step the window count and the fraction of 8 TB/s by the bytes the reference's step moves (SURVEY 8d4:
Dataset.algorithmic_bytes).  --auto adds a third handle under `amd:step = auto` and reports its decision and estimator (counters 16 / 18 / 19:
decision, estimated microseconds of the exact levels and of the stream).  One JSON line, appended to --out.

usage: python tools/wide_window.py --k 512 --items zipf --n 20000000 --out wide_window.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svdfeature_amd as sa  # noqa: E402
from benchlib import orders, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, required=True)
ap.add_argument("--items", choices=["uniform", "zipf"], default="uniform")
ap.add_argument("--pairs", action="store_true")
ap.add_argument("--n", type=int, default=20_000_000)
ap.add_argument("--users", type=int, default=200_000)
ap.add_argument("--num-items", type=int, default=20_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--auto", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()


def trainer(active, conf, extra):
    t = sa.Trainer(0, active)
    t.seed(10)
    for key, v in conf + extra:
        t.set_param(key, str(v))
    t.init_model()
    t.init_trainer()
    return t


conf = [("num_user", a.users), ("num_item", a.num_items), ("num_global", 0), ("num_factor", a.k), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004")]
if a.pairs:
    cols = synth.synth_pairs(a.n, a.users, a.num_items)
    active, conf = 3, conf + [("active_type", 3), ("no_user_bias", 1), ("base_score", "0.5")]
    build = lambda t: t.dataset_from_pairs(*cols)   # noqa: E731
else:
    class Ctx:
        Planted = synth.Planted
    cols = synth.synth_triples(a.n, a.users, a.num_items) if a.items == "uniform" else orders.synth_zipf_triples(Ctx, a.n, a.users, a.num_items, 4321)
    active, conf = 0, conf + [("base_score", "3")]
    build = lambda t: t.dataset_from_triples(*cols)   # noqa: E731
n = len(cols[0])

handles = {}
for name, extra in (("exact", []), ("window", [("amd:step", "minibatch")])):
    t = trainer(active, conf, extra)
    s = time.perf_counter()
    ds = build(t)
    t.synchronize()
    handles[name] = {"t": t, "ds": ds, "build_s": time.perf_counter() - s, "ms": []}
    t.train_dataset(ds)   # warm-up pass
    t.synchronize()
for _ in range(a.reps):
    for name in ("exact", "window"):   # alternating
        h = handles[name]
        s = time.perf_counter()
        h["t"].train_dataset(h["ds"])
        h["t"].synchronize()
        h["ms"].append(1e3 * (time.perf_counter() - s))

res = {"k": a.k, "items": "pairs" if a.pairs else a.items, "rows": n, "users": a.users, "num_items": a.num_items, "reps": a.reps}
for name, h in handles.items():
    med = float(np.median(h["ms"]))
    res[name] = {"kind": h["ds"].kind, "windows_or_levels": h["ds"].num_batches, "build_s": h["build_s"], "ms_per_pass": med, "min_ms": min(h["ms"]), "max_ms": max(h["ms"]),
                 "inst_per_s": n / med * 1e3, "frac_of_8TBps": h["ds"].algorithmic_bytes / (med * 1e-3) / 8e12,
                 "finite": bool(np.isfinite(h["t"].view("W_item")).all())}
if a.auto:
    t = trainer(active, conf, [("amd:step", "auto")])
    ds = build(t)
    res["auto"] = {"decision": t.counter(16), "levels": t.counter(17), "estimated_exact_us": t.counter(18), "estimated_stream_us": t.counter(19), "kind": ds.kind}
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""Scoring of window data sets on one MI355X (svdf_predict_dataset / svdf_eval_dataset on kinds 5, 7, 8) next to the
only way the same rows could be scored before: an exact-mode handle's level-scheduled data set (kinds 0 / 3 / 1).

  basicmf    BASELINE configs[1]: (user, item, rating), users and items uniform, k = 64 -- window sequence of kind-5 children against kind 0 / 10
  zipf       the same with items ~ Zipf(0.7) over a permuted catalogue (benchlib/orders.py) -- hot windows among the children
  svdpp      BASELINE configs[3] implicitFeedback: user blocks of --per-user rows, feedback set = own items, k = 128 -- kind-7 children against kind 3
  sidefeat   SURVEY 8(d2) side-feature variant (tools/sidefeat_window.py): 4 global ids, user + age bucket (amd:shared_user_from), item, k = 64 --
             kind-7 children with a shared user section against kind 1 / 2

Per shape: data-set build seconds (window handle and exact handle), the window handle's pass time, svdf_eval_dataset and svdf_predict_dataset as medians of --reps synchronous
calls (both end with a stream synchronisation: the wall time of a call is the time of its launches plus one copy out), inst/s and the fraction of
8 TB/s by the bytes a prediction has to move (SURVEY 8d4 without the write-back: 4k per row read, 4 per bias, the row's record).
--lib PATH loads another build of the library (the parent commit's, for build seconds and the exact rates; it refuses to score window data sets).
One JSON line per shape, appended to --out.

usage: python tools/window_scoring.py --shape basicmf --n 100000000 --out window_scoring.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import svdfeature_amd as sa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["basicmf", "zipf", "svdpp", "sidefeat"], required=True)
ap.add_argument("--n", type=int, default=0, help="rows (0 = the shape's configured size: 100 M; sidefeat: its 2 M-row prefix)")
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--per-user", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--train-passes", type=int, default=5, help="timed passes of svdf_train_dataset on the window handle")
ap.add_argument("--lib", default="", help="another libsvdfeature_amd.so to load (the parent commit's)")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.lib:
    sa.LIB_PATH = os.path.abspath(a.lib)
from benchlib import orders, synth  # noqa: E402
from svdfeature_amd import CSRData  # noqa: E402

n = a.n or (2_000_000 if a.shape == "sidefeat" else 100_000_000)
k = 128 if a.shape == "svdpp" else 64
NG, G, NB = 4, 10000, 64


def trainer(fmt, conf, extra):
    t = sa.Trainer(fmt, 0)
    t.seed(10)
    for key, v in conf + extra:
        t.set_param(key, str(v))
    t.init_model()
    t.init_trainer()
    return t


base = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("num_item", a.items), ("num_factor", k)]
t0 = time.time()
if a.shape in ("basicmf", "zipf"):
    class Ctx:
        Planted = synth.Planted
    u, i, r = synth.synth_triples(n, a.users, a.items) if a.shape == "basicmf" else orders.synth_zipf_triples(Ctx, n, a.users, a.items, 4321)
    fmt, conf, wextra = 0, base + [("num_user", a.users), ("num_global", 0)], []
    build = lambda t: t.dataset_from_triples(u, i, r)   # noqa: E731
    pred_bytes = n * (2 * 4 * k + 8 + 12)
elif a.shape == "svdpp":
    nblk = max(1, n // a.per_user)
    train, _ = synth.synth_user_blocks(nblk, a.per_user, a.users, a.items)
    n = int(train.block_row_ptr[-1])
    fmt, conf, wextra = 1, base + [("num_user", a.users), ("num_global", 0), ("num_ufeedback", a.items), ("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")], []
    build = lambda t: t.dataset_from_blocks(train)   # noqa: E731
    pred_bytes = n * (2 * 4 * k + 8 + 12) + int(train.fb_ptr[-1]) * (4 * k + 4 + 8)
else:
    rng = np.random.default_rng(1)
    uu = rng.integers(0, a.users, n, dtype=np.uint32)
    ii = rng.integers(0, a.items, n, dtype=np.uint32)
    rr = rng.integers(1, 6, n).astype(np.float32)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)
    per = NG + 3
    row_ptr = np.empty(3 * n + 1, np.int64)
    b0 = per * np.arange(n, dtype=np.int64)
    row_ptr[0:3 * n:3] = b0; row_ptr[1:3 * n:3] = b0 + NG; row_ptr[2:3 * n:3] = b0 + NG + 2; row_ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = uu; idx[:, NG + 1] = a.users + (uu % NB); idx[:, NG + 2] = ii
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    d = CSRData(rr, row_ptr.astype(np.int32), idx.ravel(), val.ravel())
    fmt, conf, wextra = 0, base + [("num_user", a.users + NB), ("num_global", G), ("wd_global", "0.001")], [("amd:shared_user_from", a.users)]
    build = lambda t: t.dataset_from_csr(d)   # noqa: E731
    pred_bytes = n * (3 * 4 * k + 3 * 4 + NG * 4 + 4 + per * 8)
gen_s = time.time() - t0


def timed(fn):
    fn()
    ts = []
    for _ in range(a.reps):
        s = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - s)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def measure(t, what):
    s = time.perf_counter()
    ds = build(t)
    t.synchronize()
    out = {"kind": ds.kind, "build_s": time.perf_counter() - s, "windows_or_levels": ds.num_batches}
    if what == "window":
        t.train_dataset(ds)   # one pass: the model is not the initial one
        t.synchronize()
        ts = []
        for _ in range(a.train_passes):   # the window step's own pass time (that training did not move: compare --lib builds)
            s = time.perf_counter()
            t.train_dataset(ds)
            t.synchronize()
            ts.append(time.perf_counter() - s)
        if ts:
            out["train_pass_ms"] = {"median": 1e3 * float(np.median(ts)), "min": 1e3 * min(ts), "max": 1e3 * max(ts)}
            out["model_checksum"] = float(np.float64(t.view("W_item")).sum())
    try:
        med, lo, hi = timed(lambda: t.eval_dataset(ds))
        ss, cnt = t.eval_dataset(ds)
        out["eval"] = {"s": med, "min_s": lo, "max_s": hi, "inst_per_s": n / med, "frac_of_8TBps": pred_bytes / med / 8e12, "rmse": float(np.sqrt(ss / cnt))}
        med, lo, hi = timed(lambda: t.predict_dataset(ds))
        out["predict"] = {"s": med, "min_s": lo, "max_s": hi, "inst_per_s": n / med}
    except sa.SvdfError as e:
        out["refused"] = str(e)[:100]
    ds.close()
    return out


res = {"shape": a.shape, "library": a.label, "rows": n, "k": k, "prediction_bytes_per_row": pred_bytes / n, "data_s": gen_s}
res["window"] = measure(trainer(fmt, conf, [("amd:step", "minibatch")] + wextra), "window")
res["exact"] = measure(trainer(fmt, conf, []), "exact")
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""SVD++ blocks with Zipf-popular items through the window step, with and without the ordered sub-steps for hot item rows (knobs
window_block_item_sub / window_block_item_max on a user-group trainer) on one MI355X.

The data are BASELINE configs[3]'s implicitFeedback shape (benchlib/synth.py: synth_user_blocks -- --per-user ratings per user, k = 128) at a
prefix of --blocks users, the items drawn Zipf(--zipf) over a random permutation of the ids the way benchlib/orders.py draws its rating stream:
  --feedback own      the demo's feedback set: the items the user rated, value n^-1/2 (Zipf-popular feedback rows as well)
  --feedback uniform  --per-user feedback ids drawn uniformly (distinct ones kept): the items alone are skewed
Paths (--paths, in the order given, alternating over --reps rounds): exact (the default step), off (window step, window_block_item_sub 0: today's
rule), hot (one path `hot<S>x<M>` per pair of --item-sub S and --item-max M; a single pair can be named directly, e.g. hot64x2048).  Per path:
windows, ms per pass as the median of the rounds with min / max, inst/s, the model checksum, counter 36 and the RMSE on the users' held-out rows
after --contract-passes passes from a fresh model (the contract |dRMSE| <= 1e-4 is against `exact` of the same build).  One JSON line, appended
to --out.

usage: python tools/block_item_hot_window.py --blocks 20000 --seed 1 --paths exact,off,hot --item-sub 64,128 --item-max 512,1024,2048,4096 --out r22.jsonl"""
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
ap.add_argument("--blocks", type=int, default=20000)
ap.add_argument("--per-user", type=int, default=100)
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--zipf", type=float, default=0.7)
ap.add_argument("--feedback", default="own", choices=["own", "uniform"])
ap.add_argument("--k", type=int, default=128)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--paths", default="exact,off,hot")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--contract-passes", type=int, default=3)
ap.add_argument("--item-sub", default="64,128", help="window_block_item_sub values of the `hot` path, comma-separated")
ap.add_argument("--item-max", default="512,1024,2048,4096", help="window_block_item_max values of the `hot` path, comma-separated")
ap.add_argument("--lib", default="")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.lib:
    sa.LIB_PATH = os.path.abspath(a.lib)
from benchlib import synth  # noqa: E402
from svdfeature_amd import BlockArrays  # noqa: E402


def zipf_user_blocks(num_blocks, per_user, num_user, num_item, seed):
    """synth_user_blocks with Zipf items: (train, held-out: the same users' feedback + 2 fresh rows, items from the same law)"""
    rng = np.random.default_rng(seed)
    users = rng.permutation(num_user)[:num_blocks].astype(np.uint32)
    w = 1.0 / np.arange(1, num_item + 1, dtype=np.float64) ** a.zipf
    cdf = np.cumsum(w / w.sum())
    perm = rng.permutation(num_item).astype(np.uint32)

    def draw(m):
        return perm[np.minimum(np.searchsorted(cdf, rng.random(m)), num_item - 1)]
    n = num_blocks * per_user
    u = np.repeat(users, per_user)
    i = draw(n)
    pl = synth.Planted(num_user, num_item, rng)
    r = pl.rate(u, i, rng)
    # feedback set of a block = its distinct items (own) or as many uniform draws, sorted, duplicates masked out (synth_user_blocks' way)
    fb = i if a.feedback == "own" else rng.integers(0, num_item, n, dtype=np.uint32)
    srt = np.sort(fb.reshape(num_blocks, per_user), axis=1)
    keep = np.ones(srt.shape, dtype=bool)
    keep[:, 1:] = srt[:, 1:] != srt[:, :-1]
    fb_idx = srt[keep].astype(np.uint32)
    fb_cnt = keep.sum(axis=1).astype(np.int64)
    fb_ptr = np.concatenate([[0], np.cumsum(fb_cnt)]).astype(np.int64)
    fb_val = (1.0 / np.sqrt(np.repeat(fb_cnt, fb_cnt))).astype(np.float32)

    def rows(uu, ii, rr, per):
        m = len(rr)
        ptr = np.empty(3 * m + 1, np.int64)
        base = 2 * np.arange(m, dtype=np.int64)
        ptr[0:3 * m:3] = base; ptr[1:3 * m:3] = base; ptr[2:3 * m:3] = base + 1; ptr[3 * m] = 2 * m
        idx = np.empty(2 * m, np.uint32); idx[0::2] = uu; idx[1::2] = ii
        return BlockArrays(np.zeros(num_blocks, np.int32), fb_ptr, fb_idx, fb_val, per * np.arange(num_blocks + 1, dtype=np.int64),
                           rr, ptr, idx, np.ones(2 * m, np.float32))
    tu = np.repeat(users, 2)
    ti = draw(len(tu))
    return rows(u, i, r, per_user), rows(tu, ti, pl.rate(tu, ti, rng), 2), i


train, test, items = zipf_user_blocks(a.blocks, a.per_user, a.users, a.items, a.seed)
n = train.num_row
conf = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("num_item", a.items), ("num_factor", a.k),
        ("num_user", a.users), ("num_global", 0), ("num_ufeedback", a.items), ("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
MB = [("amd:step", "minibatch")]
PATHS = {"exact": ([], []), "off": (MB, [])}


def hot_path(name):
    s, m = name[3:].split("x")
    return MB, [("window_block_item_sub", int(s)), ("window_block_item_max", int(m))]


def trainer(path):
    extra, knobs = PATHS[path]
    t = sa.Trainer(1, 0)
    t.seed(10)
    for kk, v in conf + extra:
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    for kk, v in knobs:
        t.set_knob(kk, v)
    return t


paths = []
for p in a.paths.split(","):
    paths += ["hot%sx%s" % (s, m) for s in a.item_sub.split(",") for m in a.item_max.split(",")] if p == "hot" else [p]
for p in paths:
    if p.startswith("hot"):
        PATHS[p] = hot_path(p)
cnt = np.bincount(items, minlength=a.items)
res = {"library": a.label, "blocks": a.blocks, "rows": n, "k": a.k, "zipf": a.zipf, "feedback": a.feedback, "seed": a.seed,
       "hottest_item_updates_per_pass": int(cnt.max()), "paths": {}}
state = {}
for p in paths:
    t = trainer(p)
    s = time.perf_counter()
    ds = t.dataset_from_blocks(train)
    t.synchronize()
    out = {"kind": ds.kind, "windows_or_levels": ds.num_batches, "build_s": time.perf_counter() - s}
    for _ in range(a.contract_passes):
        t.train_dataset(ds)
    t.synchronize()
    held = t.dataset_from_blocks(test)
    ss, c = t.eval_dataset(held)
    held.close()
    out["rmse_after_%d" % a.contract_passes] = float(np.sqrt(ss / c))
    out["model_checksum"] = float(np.float64(t.view("W_item")).sum() + np.float64(t.view("W_user")).sum())
    if p.startswith("hot"):
        out["counter_36"] = t.counter(36)
    state[p] = (t, ds, [])
    res["paths"][p] = out
for _ in range(a.reps):   # alternating rounds
    for p in paths:
        t, ds, ts = state[p]
        s = time.perf_counter()
        t.train_dataset(ds)
        t.synchronize()
        ts.append(time.perf_counter() - s)
for p in paths:
    ts = state[p][2]
    if ts:
        med = float(np.median(ts))
        res["paths"][p].update({"pass_ms": {"median": 1e3 * med, "min": 1e3 * min(ts), "max": 1e3 * max(ts)}, "inst_per_s": n / med})
if "exact" in res["paths"]:
    base = res["paths"]["exact"].get("rmse_after_%d" % a.contract_passes)
    for p, o in res["paths"].items():
        r = o.get("rmse_after_%d" % a.contract_passes)
        if base is not None and r is not None and p != "exact":
            o["abs_drmse_vs_exact"] = abs(r - base)
line = json.dumps(res)
print(line, flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(line + "\n")

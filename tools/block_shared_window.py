#!/usr/bin/env python3
"""SVD++ blocks whose rows carry a user attribute id (amd:shared_user_from on a user-group trainer) on one MI355X.

The data are BASELINE configs[3]'s implicitFeedback shape (benchlib/synth.py: synth_user_blocks -- --per-user ratings per user, feedback set = own
items, k = 128) at a prefix of --blocks users, every row carrying the user plus one attribute id `num_user + attr(user)`:
  --attr 10000   variant S: one of 10 000 sparse attribute ids per user
  --attr 64      variant D: one of 64 dense bucket ids per user
  --attr 0       no attribute: today's SVD++ window step, the ceiling
Paths (--paths, in the order given, alternating over --reps rounds): exact (the default step), general (window step, knob wunit_fast = 0),
wave (wunit_fast = 3), step (window step, default knobs: the one a library without the wave form's knob value accepts), auto (amd:step = auto:
only the decision is recorded), hot (the ordered sub-steps for hot shared user rows, DESIGN.md section 6q: one path `hot<S>x<M>` per pair of --block-sub S and
--block-max M, knobs window_block_sub / window_block_max on the default knobs otherwise; a single pair can be named directly, e.g. hot8x512).  Per path: windows, ms per pass as the median of the rounds with
min / max, inst/s, the model checksum, counters 33 / 34 / 35, and the RMSE on the users' held-out rows after --contract-passes passes from a
fresh model (the contract |dRMSE| <= 1e-4 is against `exact`).  --lib PATH loads another build of the library (the parent commit's: the only
route it has for this data is the exact pass).  --per-target-shared sets the knob window_per_target_shared.  One JSON line, appended to --out.

usage: python tools/block_shared_window.py --blocks 20000 --attr 10000 --paths exact,general,wave --out block_shared.jsonl"""
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
ap.add_argument("--attr", type=int, default=10000)
ap.add_argument("--k", type=int, default=128)
ap.add_argument("--seed", type=int, default=4242)
ap.add_argument("--paths", default="exact,general,wave")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--contract-passes", type=int, default=3)
ap.add_argument("--per-target-shared", type=int, default=0)
ap.add_argument("--block-sub", default="12", help="window_block_sub values of the `hot` path, comma-separated")
ap.add_argument("--block-max", default="512", help="window_block_max values of the `hot` path, comma-separated")
ap.add_argument("--lib", default="")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.lib:
    sa.LIB_PATH = os.path.abspath(a.lib)
from benchlib import synth  # noqa: E402
from svdfeature_amd import BlockArrays  # noqa: E402


def with_attr(ba):
    """every row's user section becomes [user, num_user + attr(user)]: an attribute of the USER (a multiplicative hash of its id)"""
    if a.attr == 0:
        return ba
    m = ba.num_row
    u, i = ba.feat_index[0::2], ba.feat_index[1::2]
    at = (a.users + (u.astype(np.uint64) * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(a.attr)).astype(np.uint32)
    idx = np.empty(3 * m, np.uint32); idx[0::3] = u; idx[1::3] = at; idx[2::3] = i
    ptr = np.empty(3 * m + 1, np.int64)
    base = 3 * np.arange(m, dtype=np.int64)
    ptr[0:3 * m:3] = base; ptr[1:3 * m:3] = base; ptr[2:3 * m:3] = base + 2; ptr[3 * m] = 3 * m
    return BlockArrays(ba.extend_tag, ba.fb_ptr, ba.fb_index, ba.fb_value, ba.block_row_ptr, ba.row_label, ptr, idx, np.ones(3 * m, np.float32))


train, test = synth.synth_user_blocks(a.blocks, a.per_user, a.users, a.items, seed=a.seed)
train, test = with_attr(train), with_attr(test)
n = train.num_row
conf = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("num_item", a.items), ("num_factor", a.k),
        ("num_user", a.users + a.attr), ("num_global", 0), ("num_ufeedback", a.items), ("wd_ufeedback", "0.004"), ("ufeedback_init_sigma", "0.01")]
key = [("amd:shared_user_from", a.users)] if a.attr else []
PATHS = {"exact": ([], []), "general": ([("amd:step", "minibatch")] + key, [("wunit_fast", 0)]), "wave": ([("amd:step", "minibatch")] + key, [("wunit_fast", 3)]),
         "step": ([("amd:step", "minibatch")] + key, []), "auto": ([("amd:step", "auto")] + key, [])}


def hot_path(name):
    s, m = name[3:].split("x")
    return [("amd:step", "minibatch")] + key, [("window_block_sub", int(s)), ("window_block_max", int(m))]


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
    if a.per_target_shared and extra:
        t.set_knob("window_per_target_shared", a.per_target_shared)
    return t


paths = []
for p in a.paths.split(","):
    paths += ["hot%sx%s" % (s, m) for s in a.block_sub.split(",") for m in a.block_max.split(",")] if p == "hot" else [p]
for p in paths:
    if p.startswith("hot"):
        PATHS[p] = hot_path(p)
res = {"library": a.label, "blocks": a.blocks, "rows": n, "k": a.k, "attr": a.attr, "seed": a.seed, "per_target_shared": a.per_target_shared or 12, "paths": {}}
state = {}
for p in paths:
    t = trainer(p)
    s = time.perf_counter()
    ds = t.dataset_from_blocks(train)
    t.synchronize()
    out = {"kind": ds.kind, "windows_or_levels": ds.num_batches, "build_s": time.perf_counter() - s, "auto_decision": t.counter(16)}
    if p != "auto":
        for _ in range(a.contract_passes):
            t.train_dataset(ds)
        t.synchronize()
        try:
            held = t.dataset_from_blocks(test)
            ss, cnt = t.eval_dataset(held)
            held.close()
            out["rmse_after_%d" % a.contract_passes] = float(np.sqrt(ss / cnt))
        except sa.SvdfError as e:   # (the parent's library does not score window data sets)
            out["rmse_refused"] = str(e)[:80]
        out["model_checksum"] = float(np.float64(t.view("W_item")).sum() + np.float64(t.view("W_user")).sum())
        out["counter_33_34"] = [t.counter(33), t.counter(34)]
        if p.startswith("hot"):
            out["counter_35"] = t.counter(35)
    state[p] = (t, ds, [])
    res["paths"][p] = out
for _ in range(a.reps):   # alternating rounds
    for p in paths:
        if p == "auto":
            continue
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

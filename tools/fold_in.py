#!/usr/bin/env python3
"""Fold-in on the live model (svdf_fold_in) against the only route the parent has to the same rows: Trainer.view("W_item"),
then a batched float32 solve in numpy on the host.  Results in profiles/r48_fold_in.md.

Input: --users sections (10 000) of --ratings ratings (100) each over --items items (100 000) at one num_factor per invocation; a random
normal model written with set_view.  The two routes alternate --reps times (5) after a warm-up of each; medians with min .. max.  Three more
shapes of the same call say which part of the kernel binds: `same_item` (every rating names item 0: the gather comes from cache, Gram sum and
factorisation stay), `one_rating` (a section is one rating: the factorisation and the call's fixed cost stay).

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/fold_in.py --k 64 --out r48_k64.json && timeout -k 10 300 python tools/fold_in.py --k 128 --out r48_k128.json

--only-call runs svdf_fold_in on the three shapes --reps times after a warm-up: the program to put behind `rocprofv3 --kernel-trace --stats --`
in a run of its own (the shapes are then the kernel's launches 2 .. reps + 1 of each group, in that order)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def host_route(t, users, item, label, reg, base, R):
    """the parent's route: the item side copied out, A and b of every section by batched float32 matmuls, numpy.linalg.solve on the stack"""
    W, ib, ub = t.view("W_item"), t.view("i_bias"), t.view("u_bias")
    Q = W[item].reshape(len(users), R, -1)
    y = (label - (np.float32(base) + np.repeat(ub[users], R) + ib[item])).reshape(len(users), R, 1)
    A = np.matmul(Q.transpose(0, 2, 1), Q) + np.float32(reg) * np.eye(Q.shape[2], dtype=np.float32)
    return np.linalg.solve(A, np.matmul(Q.transpose(0, 2, 1), y))[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--users", type=int, default=10000)
    ap.add_argument("--ratings", type=int, default=100)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--reg", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-call", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    S, R, ni, k = a.users, a.ratings, a.items, a.k
    t = sa.Trainer(0, 0)
    t.seed(7)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=S, num_item=ni, num_factor=k):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    rng = np.random.default_rng(11)
    t.set_view("W_item", rng.standard_normal((ni, k)).astype(np.float32))
    t.set_view("i_bias", rng.standard_normal(ni).astype(np.float32))
    t.set_view("u_bias", rng.standard_normal(S).astype(np.float32))
    users = np.arange(S, dtype=np.uint32)
    item = rng.integers(0, ni, S * R).astype(np.uint32)
    label = rng.standard_normal(S * R).astype(np.float32) + np.float32(3)
    ptr = R * np.arange(S + 1, dtype=np.int64)
    shapes = {"full": lambda: t.fold_in(users, ptr, item, label, a.reg),
              "same_item": lambda: t.fold_in(users, ptr, np.zeros_like(item), label, a.reg),
              "one_rating": lambda: t.fold_in(users, np.arange(S + 1, dtype=np.int64), item[:S], label[:S], a.reg)}
    rec = {"k": k, "users": S, "ratings": R, "items": ni, "reg": a.reg, "reps": a.reps}
    if a.only_call:
        for f in shapes.values():
            for _ in range(a.reps + 1):
                f()
    else:
        routes = dict(shapes, host=lambda: host_route(t, users, item, label, a.reg, 3.0, R))
        got = {name: f() for name, f in routes.items()}   # warm-up of each: buffers, code objects
        secs = {name: [] for name in routes}
        for _ in range(a.reps):
            for name, f in routes.items():
                t0 = time.perf_counter()
                f()
                secs[name].append(time.perf_counter() - t0)
        for name in routes:
            rec[name + "_s"] = spread(secs[name])
        rec["host_over_call"] = float(np.median(secs["host"]) / np.median(secs["full"]))
        err = np.linalg.norm(got["full"] - got["host"], axis=1) / np.linalg.norm(got["host"], axis=1)
        rec["largest_relative_difference_from_host_route"] = float(err.max())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

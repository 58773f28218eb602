#!/usr/bin/env python3
"""Similar-item lists on the live model (svdf_item_topn) against (a) the parent's sweep -- svdf_rank_topn over the
same number of sections without bans, in the same build: an item call should cost that sweep plus its two small kernels -- and (b) the
route a user has today on the same GPU: torch, Q @ W.T in row chunks, the query masked, torch.topk (its rounding differs, so it gives
time only).  Results in profiles/r40_item_topn.md.

Input: tools/rank_topn.py's model -- --items items (100 000) at one num_factor per invocation, trained by one pass of rank pairs first.
For every top_n of --top (10,100), both metrics and every query count of --queries (10000,all): the three routes alternate --reps times
(5) on the same queries after a warm-up of each; medians with min .. max are reported.  The torch route is timed with W already on the
device and includes the copy of ids and scores to the host, as the item call does.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 600 python tools/item_topn.py --k 64 --out r40_k64.json && timeout -k 10 600 python tools/item_topn.py --k 128 --out r40_k128.json

--only-batch runs svdf_item_topn (first top_n of --top, first query count, both metrics) --reps times after a warm-up: the program to put
behind `rocprofv3 --kernel-trace --stats --` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

METRICS = ("dot", "cosine")


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def torch_route(torch, Wd, q, top_n, metric, chunk=4096):
    """today's route: (cosine: normalise,) Q @ W.T in row chunks, the query masked, topk; ids and scores copied to the host"""
    base = Wd / Wd.norm(dim=1, keepdim=True).clamp_min(1e-30) if metric == "cosine" else Wd
    ids, scores = [], []
    for a in range(0, len(q), chunk):
        qq = q[a:a + chunk]
        sc = base[qq] @ base.T
        sc[torch.arange(len(qq), device=sc.device), qq] = float("-inf")
        v, i = torch.topk(sc, top_n, dim=1)
        ids.append(i)
        scores.append(v)
    return torch.cat(ids).cpu().numpy(), torch.cat(scores).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
    ap.add_argument("--queries", default="10000,all")
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    nu, ni, k = a.users, a.items, a.k
    tops = [int(x) for x in a.top.split(",")]
    counts = [ni if x == "all" else int(x) for x in a.queries.split(",")]
    t = sa.Trainer(0, 3)
    t.seed(7)
    for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(1000000, nu, ni, seed=3)))
    t.synchronize()
    rng = np.random.default_rng(11)
    rec = {"k": k, "items": ni, "reps": a.reps, "runs": []}
    if a.only_batch:
        S, N = counts[0], tops[0]
        q = np.arange(ni, dtype=np.uint32) if S == ni else rng.permutation(ni)[:S].astype(np.uint32)
        for metric in METRICS:
            t.similar_items(q, N, metric)
            secs = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                t.similar_items(q, N, metric)
                secs.append(time.perf_counter() - t0)
            rec["runs"].append({"queries": S, "top_n": N, "metric": metric, "item_s": spread(secs)})
    else:
        torch = Wd = None
        if not a.no_torch:
            import torch
            Wd = torch.from_numpy(t.view("W_item").copy()).to("cuda")
        for S in counts:
            q = np.arange(ni, dtype=np.uint32) if S == ni else rng.permutation(ni)[:S].astype(np.uint32)
            users = rng.integers(0, nu, S).astype(np.uint32)
            qd = torch.from_numpy(q.astype(np.int64)).to("cuda") if torch else None
            for N in tops:
                for metric in METRICS:
                    routes = {"item": lambda: t.similar_items(q, N, metric), "sweep": lambda: t.rank_topn(users, N)}
                    if torch:
                        routes["torch"] = lambda: torch_route(torch, Wd, qd, N, metric)
                    got = {name: f() for name, f in routes.items()}          # warm-up of each: buffers, code objects
                    secs = {name: [] for name in routes}
                    for _ in range(a.reps):
                        for name, f in routes.items():
                            t0 = time.perf_counter()
                            f()
                            secs[name].append(time.perf_counter() - t0)
                    run = {"queries": S, "top_n": N, "metric": metric, "nan_sections": int(got["item"][3].sum())}
                    for name in routes:
                        run[name + "_s"] = spread(secs[name])
                    run["item_over_sweep"] = float(np.median(secs["item"]) / np.median(secs["sweep"]))
                    if torch:
                        run["torch_over_item"] = float(np.median(secs["torch"]) / np.median(secs["item"]))
                        run["same_ids_as_torch"] = float((got["item"][0] == got["torch"][0]).mean())   # (roundings differ: a figure, not a check)
                    rec["runs"].append(run)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The two scoring modes of the top-N sweeps (knob rank_topn_scores) side by side: 0, the pinned sweeps, and 1, the
sweep on the matrix cores (svdf_k_ranktopn_mfma.hip), on one trainer whose model is random normal rows written with set_view; next to them
the torch comparator of tools/item_topn.py.  Results in profiles/r41_rank_matrix.md.

For every top_n of --top and every call of --calls (rank_topn, dot, cosine) the routes alternate --reps times (5) after a warm-up of each;
medians with min .. max of the host clock around the call, which ends in a synchronise.  --sections all: every item is a query (item calls
only).  Accuracy: for --sample seeded sections of the rank_topn call, the largest |score - float64 score| / bound of the published
contract over the listed items.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_matrix.py --k 64 --out r41_k64.json && timeout -k 10 300 python tools/rank_matrix.py --k 128 --out r41_k128.json

--tables a.json b.json ... prints the records of earlier runs as the markdown table of the note, and uses no GPU.

--only-batch runs rank_topn under knob 1 (first top_n) --reps times after a warm-up: the program to put behind
`rocprofv3 --kernel-trace --stats --` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def error_ratio(got, U, W, bias, k):
    """largest |error| / bound over the listed items of the sections whose effective rows are U"""
    worst = 0.0
    for s in range(len(U)):
        ids = got[0][s][:got[2][s]].astype(np.int64)
        u, v, b = U[s].astype(np.float64), W[ids].astype(np.float64), bias[ids].astype(np.float64)
        bound = 2.0 * (k + 2) * 2.0 ** -24 * (np.abs(b) + np.abs(v) @ np.abs(u))
        worst = max(worst, float((np.abs(got[1][s][:len(ids)].astype(np.float64) - (b + v @ u)) / bound).max(initial=0.0)))
    return worst


def tables(paths):
    """the markdown table of profiles/r41_rank_matrix.md from the JSON records of earlier runs: milliseconds, median (min .. max)"""
    ms = lambda x: "%.2f (%.2f .. %.2f)" % (1e3 * x["median"], 1e3 * x["min"], 1e3 * x["max"]) if x else "--"
    print("| k | sections | call | top_n | pinned | matrix | torch | pinned / matrix | error / bound |")
    print("|---|---|---|---|---|---|---|---|---|")
    for path in paths:
        with open(path) as f:
            rec = json.loads(f.readline())
        for r in rec["runs"]:
            err = "%.4f" % r["error_over_bound"] if "error_over_bound" in r else "--"
            print("| %d | %d | %s | %d | %s | %s | %s | %.2f | %s |" % (rec["k"], rec["sections"], r["call"], r["top_n"], ms(r["pinned_s"]), ms(r["matrix_s"]),
                                                                  ms(r.get("torch_s")), r["pinned_over_matrix"], err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", default=None, help="JSON records of earlier runs: print the note's table and exit")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
    ap.add_argument("--sections", default="10000")
    ap.add_argument("--calls", default="rank_topn,dot,cosine")
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    if a.tables:
        return tables(a.tables)
    import cases
    import svdfeature_amd as sa
    from item_topn import spread, torch_route
    nu, ni, k = a.users, a.items, a.k
    S = ni if a.sections == "all" else int(a.sections)
    tops = [int(x) for x in a.top.split(",")]
    t = sa.Trainer(0, 0)
    t.seed(7)
    for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    rng = np.random.default_rng(11)
    U, W = rng.standard_normal((nu, k), np.float32), rng.standard_normal((ni, k), np.float32)
    bias = rng.standard_normal(ni, np.float32)
    for name, v in (("W_user", U), ("W_item", W), ("i_bias", bias)):
        t.set_view(name, v)
    q = np.arange(ni, dtype=np.uint32) if S == ni else rng.permutation(ni)[:S].astype(np.uint32)
    users = rng.integers(0, nu, S).astype(np.uint32)

    def call(name, N, knob):
        t.set_knob("rank_topn_scores", knob)
        return t.rank_topn(users, N) if name == "rank_topn" else t.similar_items(q, N, name)

    rec = {"k": k, "items": ni, "sections": S, "reps": a.reps, "runs": []}
    if a.only_batch:
        call("rank_topn", tops[0], 1)
        secs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call("rank_topn", tops[0], 1)
            secs.append(time.perf_counter() - t0)
        rec["runs"].append({"call": "rank_topn", "top_n": tops[0], "matrix_s": spread(secs)})
    else:
        torch = Wd = qd = None
        if not a.no_torch:
            import torch
            Wd, qd = torch.from_numpy(W).to("cuda"), torch.from_numpy(q.astype(np.int64)).to("cuda")
        for name in a.calls.split(","):
            for N in tops:
                routes = {"pinned": lambda: call(name, N, 0), "matrix": lambda: call(name, N, 1)}
                if torch and name != "rank_topn":
                    routes["torch"] = lambda: torch_route(torch, Wd, qd, N, name)
                got = {r: f() for r, f in routes.items()}          # warm-up of each: buffers, code objects
                secs = {r: [] for r in routes}
                for _ in range(a.reps):
                    for r, f in routes.items():
                        t0 = time.perf_counter()
                        f()
                        secs[r].append(time.perf_counter() - t0)
                run = {"call": name, "top_n": N, "same_ids": float((got["pinned"][0] == got["matrix"][0]).mean())}
                for r in routes:
                    run[r + "_s"] = spread(secs[r])
                run["pinned_over_matrix"] = float(np.median(secs["pinned"]) / np.median(secs["matrix"]))
                if name == "rank_topn":
                    pick = np.random.default_rng(5).permutation(S)[:a.sample]
                    run["error_over_bound"] = error_ratio([x[pick] for x in got["matrix"]], U[users[pick]], W, bias, k)
                rec["runs"].append(run)
    t.set_knob("rank_topn_scores", 0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

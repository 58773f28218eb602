#!/usr/bin/env python3
"""The three ways to a top-N list side by side: the pinned sweeps, the pinned lists through the certified
matrix-core prefilter (knob rank_topn_prefilter = 1, svdf_k_ranktopn_exact.hip) and -- as the floor, not as a target -- the matrix sweep
alone (knob rank_topn_scores = 1, section 6ah), on one trainer whose model is random normal rows written with set_view.  Results in
profiles/r43_rank_prefilter.md.

For every top_n of --top and every call of --calls (rank_topn, dot, cosine) the three modes alternate --reps times (5) after a warm-up of
each; medians with min .. max of the host clock around the call, which ends in a synchronise.  --sections all: every item is a query
(item calls only).  Per cell: whether every prefilter list equals the pinned list (ids, score bits, counts, flags) and the share of the
sections the pinned sweep listed again (counter 52) at --slack.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_prefilter.py --k 64 --out r43_k64.json && timeout -k 10 300 python tools/rank_prefilter.py --k 128 --out r43_k128.json

--tables a.json b.json ... prints the records of earlier runs as the markdown table of the note, and uses no GPU.

--only-batch runs rank_topn under the prefilter (first top_n) --reps times after a warm-up: the program to put behind
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

MODES = {"pinned": (0, 0), "prefilter": (0, 1), "matrix": (1, 0)}   # (rank_topn_scores, rank_topn_prefilter)


def tables(paths):
    """the markdown table of profiles/r43_rank_prefilter.md from the JSON records of earlier runs: milliseconds, median (min .. max)"""
    ms = lambda x: "%.2f (%.2f .. %.2f)" % (1e3 * x["median"], 1e3 * x["min"], 1e3 * x["max"])
    print("| k | sections | call | top_n | pinned | prefilter | matrix (floor) | pinned / prefilter | listed again | lists equal |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for path in paths:
        with open(path) as f:
            rec = json.loads(f.readline())
        for r in rec["runs"]:
            print("| %d | %d | %s | %d | %s | %s | %s | %.2f | %.2f %% | %s |" % (rec["k"], rec["sections"], r["call"], r["top_n"], ms(r["pinned_s"]),
                                                                             ms(r["prefilter_s"]), ms(r["matrix_s"]), r["pinned_over_prefilter"],
                                                                             100.0 * r["listed_again"], "yes" if r["lists_equal"] else "NO"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", default=None, help="JSON records of earlier runs: print the note's table and exit")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
    ap.add_argument("--sections", default="10000")
    ap.add_argument("--calls", default="rank_topn")
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slack", type=int, default=32)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    if a.tables:
        return tables(a.tables)
    import cases
    import svdfeature_amd as sa
    from item_topn import spread
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
    t.set_knob("rank_topn_prefilter_slack", a.slack)
    q = np.arange(ni, dtype=np.uint32) if S == ni else rng.permutation(ni)[:S].astype(np.uint32)
    users = rng.integers(0, nu, S).astype(np.uint32)

    def call(name, N, mode):
        t.set_knob("rank_topn_scores", MODES[mode][0])
        t.set_knob("rank_topn_prefilter", MODES[mode][1])
        return t.rank_topn(users, N) if name == "rank_topn" else t.similar_items(q, N, name)

    rec = {"k": k, "items": ni, "sections": S, "reps": a.reps, "slack": a.slack, "runs": []}
    if a.only_batch:
        call("rank_topn", tops[0], "prefilter")
        secs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call("rank_topn", tops[0], "prefilter")
            secs.append(time.perf_counter() - t0)
        rec["runs"].append({"call": "rank_topn", "top_n": tops[0], "prefilter_s": spread(secs)})
    else:
        for name in a.calls.split(","):
            for N in tops:
                again = t.counter(52)
                got = {m: call(name, N, m) for m in MODES}          # warm-up of each: buffers, code objects
                again = t.counter(52) - again
                secs = {m: [] for m in MODES}
                for _ in range(a.reps):
                    for m in MODES:
                        t0 = time.perf_counter()
                        call(name, N, m)
                        secs[m].append(time.perf_counter() - t0)
                equal = all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(got["prefilter"], got["pinned"]))
                run = {"call": name, "top_n": N, "lists_equal": bool(equal), "listed_again": again / S}
                for m in MODES:
                    run[m + "_s"] = spread(secs[m])
                run["pinned_over_prefilter"] = float(np.median(secs["pinned"]) / np.median(secs["prefilter"]))
                rec["runs"].append(run)
    t.set_knob("rank_topn_scores", 0)
    t.set_knob("rank_topn_prefilter", 0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rank positions by the pinned sweep and through the certified counting sweep on the matrix cores side by side (knob rank_eval_prefilter,
svdf_k_rankeval_mfma.hip), on one trainer whose model is random normal rows written with set_view.  Results in
profiles/r44_rank_eval_prefilter.md.

The two knob values alternate --reps times (5) after a warm-up of each; medians with min .. max of the host clock around the call, which
ends in a synchronise.  Per cell: whether all four outputs are equal, the sections the pinned sweep ranked again (counter 54), and the mean
and the largest band length of a row (counters 55 .. 57) at the capacity --band.  --feedback: a user-group trainer, three feedback entries
per section.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_eval_prefilter.py --k 64 --out r44_k64.json && timeout -k 10 300 python tools/rank_eval_prefilter.py --k 128 --out r44_k128.json

--tables a.json b.json ... prints the records of earlier runs as the markdown table of the note, and uses no GPU.

--only-batch runs the knob-1 call --reps times after a warm-up: the program to put behind `rocprofv3 --kernel-trace --stats --` in a run
of its own."""
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


def tables(paths):
    ms = lambda x: "%.2f (%.2f .. %.2f)" % (1e3 * x["median"], 1e3 * x["min"], 1e3 * x["max"])
    print("| k | sections | positives | route | knob 0 | knob 1 | knob 0 / knob 1 | band mean | band max | ranked again | outputs equal |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for path in paths:
        with open(path) as f:
            r = json.loads(f.readline())
        print("| %d | %d | %d | %s | %s | %s | %.2f | %.1f | %d | %d | %s |" % (r["k"], r["sections"], r["positives"], r["route"], ms(r["knob0_s"]), ms(r["knob1_s"]),
                                                                            r["knob0_over_knob1"], r["band_mean"], r["band_max"], r["ranked_again"],
                                                                            "yes" if r["outputs_equal"] else "NO"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", nargs="+", default=None, help="JSON records of earlier runs: print the note's table and exit")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--sections", type=int, default=10000)
    ap.add_argument("--positives", type=int, default=3)
    ap.add_argument("--bans", type=int, default=100)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band", type=int, default=1024)
    ap.add_argument("--budget", type=int, default=0, help="rank_eval_budget; 0: the default")
    ap.add_argument("--feedback", action="store_true")
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    if a.tables:
        return tables(a.tables)
    import cases
    import svdfeature_amd as sa
    from item_topn import spread
    nu, ni, k, S = a.users, a.items, a.k, a.sections
    rng = np.random.default_rng(11)
    if a.feedback:
        from test_rank_feedback import NFB, fb_conf
        t = sa.Trainer(1, 0)
        conf = fb_conf(nu, ni, k)
    else:
        t = sa.Trainer(0, 0)
        conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k)
    t.seed(7)
    for kk, v in conf:
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    for name, v in (("W_user", rng.standard_normal((nu, k), np.float32)), ("W_item", rng.standard_normal((ni, k), np.float32)),
                    ("i_bias", rng.standard_normal(ni, np.float32))):
        t.set_view(name, v)
    extra = {}
    if a.feedback:
        t.set_view("W_ufeedback", rng.standard_normal((NFB, k), np.float32))
        extra["feedback"] = (np.arange(0, 3 * S + 1, 3, dtype=np.int64), rng.integers(0, NFB, 3 * S).astype(np.uint32), rng.standard_normal(3 * S).astype(np.float32))
    t.set_knob("rank_eval_prefilter_band", a.band)
    if a.budget:
        t.set_knob("rank_eval_budget", a.budget)
    per = a.positives + a.bans
    pick = np.stack([rng.choice(ni, per, replace=False) for _ in range(S)]).astype(np.uint32)
    lists = (rng.integers(0, nu, S).astype(np.uint32), a.positives * np.arange(S + 1, dtype=np.int64), pick[:, :a.positives].ravel(),
             a.bans * np.arange(S + 1, dtype=np.int64), pick[:, a.positives:].ravel())

    def call(knob):
        t.set_knob("rank_eval_prefilter", knob)
        return t.rank_positions(*lists, **extra)

    rec = {"k": k, "items": ni, "sections": S, "positives": a.positives, "bans": a.bans, "reps": a.reps, "band": a.band, "budget": a.budget, "route": "feedback" if a.feedback else "plain"}
    before = [t.counter(c) for c in (54, 55, 56)]
    got = {knob: call(knob) for knob in ((1,) if a.only_batch else (0, 1))}   # warm-up of each: buffers, code objects
    again, rows, ids = [t.counter(c) - b for c, b in zip((54, 55, 56), before)]
    secs = {knob: [] for knob in got}
    for _ in range(a.reps):
        for knob in got:
            t0 = time.perf_counter()
            call(knob)
            secs[knob].append(time.perf_counter() - t0)
    rec.update(ranked_again=again, band_mean=ids / max(rows, 1), band_max=t.counter(57), knob1_s=spread(secs[1]))
    if not a.only_batch:
        rec.update(knob0_s=spread(secs[0]), knob0_over_knob1=float(np.median(secs[0]) / np.median(secs[1])),
                   outputs_equal=bool(all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))))
    t.set_knob("rank_eval_prefilter", 0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

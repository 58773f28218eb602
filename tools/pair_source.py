#!/usr/bin/env python3
"""Round loop of pairwise training from positives only on one GPU (results in profiles/r33_pair_source.md): a round is
build + train + synchronize + destroy of one pass of rank pairs, and two routes to the same pass alternate in one process, round by round:

    source    Trainer.dataset_from_pair_source(src, num_neg, seed): the negatives are drawn on the device, the pass is built from the columns in HBM
    host      pair_negatives(...) on the host (timed on its own), then Trainer.dataset_from_pairs(user, pos, neg): the only route before the source

on two trainers started from the same model file.  After EVERY round the models of the two are compared bit for bit; a difference ends the run.
The source is section 6v's shape: --users x --items, --rows positives in shuffled order, num_factor --factor.  Two configurations, a process
each: the exact pass (no amd:step) and `amd:step = minibatch`.

    python tools/pair_source.py                                   # both configurations: medians of --rounds rounds with min .. max, one JSON line each
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pair_source.py --child --config exact --only source --rounds 2
                                                                  # k_pair_draw's own time against the pass's other kernels, in a run of its own

One more round runs first and is not counted (first launches, the window rule's first search)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = ("W_user", "W_item", "i_bias")
C_HBM, C_FALLBACK = 44, 45


def rows(a):
    """--rows positives in shuffled order; every user draws from its own half of the items, so a user's distinct positives stay far below the density limit"""
    rng = np.random.default_rng(a.seed)
    u = rng.integers(0, a.users, a.rows).astype(np.uint32)
    p = ((u.astype(np.int64) * 7919 + rng.integers(0, a.items // 2, a.rows)) % a.items).astype(np.uint32)
    return u, p


def trainer(sa, a, model):
    t = sa.Trainer(0, 3)
    t.seed(10)
    conf = [("num_user", a.users), ("num_item", a.items), ("num_global", 0), ("num_factor", a.factor), ("base_score", 0.5), ("learning_rate", 0.005),
            ("wd_user", 0.004), ("wd_item", 0.004), ("active_type", 3), ("no_user_bias", 1)]
    if a.config == "minibatch":
        conf.append(("amd:step", "minibatch"))
    for k, v in conf:
        t.set_param(k, str(v))
    if model and os.path.exists(model):
        t.load_model(model)
    else:
        t.init_model()
    t.init_trainer()
    return t


def timed_round(t, build):
    """(build, train, destroy, round) seconds, the data set's (kind, info(8), windows or levels, rows)"""
    t.synchronize()
    t0 = time.perf_counter()
    ds = build()
    t.synchronize()
    t1 = time.perf_counter()
    t.train_dataset(ds)
    t.synchronize()
    t2 = time.perf_counter()
    shape = [ds.kind, ds.info(8), ds.num_batches, ds.num_row]
    ds.close()
    t.synchronize()
    t3 = time.perf_counter()
    return {"build_s": t1 - t0, "train_s": t2 - t1, "destroy_s": t3 - t2, "round_s": t3 - t0}, shape


def child(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    m = a.num_neg
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a, None)
        t0.save_model(model)
        t0.close()
        A = trainer(sa, a, model) if a.only in ("both", "source") else None
        B = trainer(sa, a, model) if a.only in ("both", "host") else None
    out = {"config": a.config, "users": a.users, "items": a.items, "rows": a.rows, "factor": a.factor, "num_neg": m, "source": [], "host": [], "host_draw_s": [],
           "device_draw_call_s": [], "shapes": {}, "models_equal": []}
    if A:
        c0 = time.perf_counter()
        src = A.pair_source(u, p)
        A.synchronize()
        out["source_create_s"] = time.perf_counter() - c0
    ru, rp = (np.repeat(u, m), np.repeat(p, m)) if m > 1 else (u, p)
    for r in range(a.rounds + 1):
        seed = a.seed + 1000 + r
        order = ("source", "host") if r % 2 == 0 else ("host", "source")   # the two alternate, and so does who goes first
        for who in order:
            if who == "source" and A:
                res, shape = timed_round(A, lambda: A.dataset_from_pair_source(src, m, seed))
            elif who == "host" and B:
                h0 = time.perf_counter()
                neg = sa.pair_negatives(a.users, a.items, u, p, m, seed)
                res = {"host_draw_s": time.perf_counter() - h0}
                tm, shape = timed_round(B, lambda: B.dataset_from_pairs(ru, rp, neg))
                res.update(tm)
                res["round_with_draw_s"] = res["round_s"] + res["host_draw_s"]
            else:
                continue
            out["shapes"][who] = shape
            if r > 0:
                out[who].append(res)
        if A and B:
            same = all(np.array_equal(A.view(v).view(np.uint32), B.view(v).view(np.uint32)) for v in VIEWS)
            out["models_equal"].append(bool(same))
            if not same:
                print("RESULT " + json.dumps(out), flush=True)
                raise SystemExit("round %d: the models of the two routes differ" % r)
            assert out["shapes"]["source"] == out["shapes"]["host"], out["shapes"]
        if A and r > 0:   # the draw on its own: kernel + the negative column's copy to the host (an upper bound of the kernel; its own time: rocprofv3)
            d0 = time.perf_counter()
            A.pair_source_draw(src, m, seed)
            out["device_draw_call_s"].append(time.perf_counter() - d0)
    if A:
        out["counters"] = {str(c): A.counter(c) for c in (C_HBM, C_FALLBACK)}
        src.close()
        A.close()
    if B:
        B.close()
    print("RESULT " + json.dumps(out), flush=True)


def med(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]} if x else None


def column(rs, key):
    return med([r[key] for r in rs if key in r])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--factor", type=int, default=128)
    ap.add_argument("--num-neg", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per route (one more runs first)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--config", default="both", choices=["both", "exact", "minibatch"])
    ap.add_argument("--only", default="both", choices=["both", "source", "host"], help="--child: one route alone (a profiler's run)")
    ap.add_argument("--child-timeout", type=int, default=500)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    for config in (["exact", "minibatch"] if a.config == "both" else [a.config]):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--config", config, "--users", str(a.users), "--items", str(a.items), "--rows", str(a.rows),
               "--factor", str(a.factor), "--num-neg", str(a.num_neg), "--rounds", str(a.rounds), "--seed", str(a.seed)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
        got = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            raise SystemExit("child failed (%d): %s\n%s\n%s" % (p.returncode, " ".join(cmd), "\n".join(got), p.stderr[-2000:]))
        r = json.loads(got[-1][7:])
        assert all(r["models_equal"]) and len(r["models_equal"]) == a.rounds + 1
        line = {"what": "round", "config": config, "pairs_per_pass": a.rows * a.num_neg, "shape": r["shapes"]["source"], "counters": r["counters"],
                "models_equal_in_every_round": True, "source_create_s": r["source_create_s"],
                "source": {k: column(r["source"], k) for k in ("round_s", "build_s", "train_s", "destroy_s")},
                "host": {k: column(r["host"], k) for k in ("round_with_draw_s", "host_draw_s", "round_s", "build_s", "train_s", "destroy_s")},
                "device_draw_call_s": med(r["device_draw_call_s"])}
        s, h = line["source"]["round_s"], line["host"]["round_with_draw_s"]
        line["ratio_of_medians"] = h["median"] / s["median"]
        line["exceeds_both_spreads"] = bool(s["max"] < h["min"])   # every round of the source faster than every round of the host route
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Item-weighted negatives for pair-source passes on one GPU (results in profiles/r36_pair_weight.md).  Measurements,
each a process of its own printing JSON lines:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pair_weight.py draws --plan PLAN [--items 10000]
    python tools/pair_weight.py trace DIR --plan PLAN
        the kernels' own time: `draws` only calls pair_source_draw -- per weight table (Zipf(0.7) counts to the 0.75; all equal) the uniform
        source, the weighted source in form 1 and in form 2, ALTERNATING call by call, --rounds times after one uncounted call each, first
        the plain draw (k_pair_draw), then hard=--cand (k_pair_hard) -- under the profiler, and writes the order of its calls to PLAN;
        `trace` reads the dispatches of DIR's kernel trace in that order and prints per cell the median time with min .. max
    python tools/pair_weight.py rounds [--config exact|minibatch] [--items 10000]
        round time (build + train + synchronize + destroy) on three trainers started from one model file, alternating round by round: the
        uniform source; the weighted source; and the only route to the same negatives without it -- pair_negatives(item_weight=) on the host,
        then dataset_from_pairs -- whose host draw is timed apart.  The weighted and the host route are asserted to train equal models.
    python tools/pair_weight.py quality [--learning-rate 0.02]
        a planted implicit-feedback set with Zipf(0.7) item popularity, a tenth of the positives held out: MAP and AUC of
        rank_eval(..., sampled=(99, seed)) after --rounds rounds from one cold start with uniform / weighted (count^0.75) negatives, plain
        and hard=8.  Reported, not asserted.

The source is section 6ac's shape: --users x --items, --rows positives in shuffled order."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTERS = (44, 45, 46, 47)
VIEWS = ("W_user", "W_item", "i_bias")


def rows(a):
    """--rows positives in shuffled order; every user draws from its own half of the items (tools/pair_source.py's source)"""
    rng = np.random.default_rng(a.seed)
    u = rng.integers(0, a.users, a.rows).astype(np.uint32)
    p = ((u.astype(np.int64) * 7919 + rng.integers(0, a.items // 2, a.rows)) % a.items).astype(np.uint32)
    return u, p


def weight_tables(a):
    """name -> uint32[items]: Zipf(0.7) counts summing to --rows, to the 0.75, on the largest power-of-two scale that keeps the sum below
    2^31, the popular ids scattered over the catalogue; and all equal"""
    rank = np.random.default_rng(a.seed + 5).permutation(a.items)
    count = (rank + 1.0) ** -0.7
    count *= a.rows / count.sum()
    w = count ** 0.75
    scale = 2.0 ** np.floor(np.log2((1 << 31) / w.sum()))
    return {"zipf": np.maximum(np.rint(scale * w), 1).astype(np.uint32), "equal": np.ones(a.items, np.uint32)}


def trainer(sa, a, model=None, users=None, items=None):
    t = sa.Trainer(0, 3)
    t.seed(10)
    conf = [("num_user", users or a.users), ("num_item", items or a.items), ("num_global", 0), ("num_factor", a.factor), ("base_score", 0.5),
            ("learning_rate", a.learning_rate), ("wd_user", 0.004), ("wd_item", 0.004), ("active_type", 3), ("no_user_bias", 1)]
    if a.config == "minibatch":
        conf.append(("amd:step", "minibatch"))
    for k, v in conf:
        t.set_param(k, str(v))
    if model:
        t.load_model(model)
    else:
        t.init_model()
    t.init_trainer()
    return t


def timed_round(t, build):
    t.synchronize()
    t0 = time.perf_counter()
    ds = build()
    t.synchronize()
    t1 = time.perf_counter()
    t.train_dataset(ds)
    t.synchronize()
    t2 = time.perf_counter()
    shape = [ds.kind, ds.info(8), ds.num_row]
    ds.close()
    t.synchronize()
    t3 = time.perf_counter()
    return {"build_s": t1 - t0, "train_s": t2 - t1, "destroy_s": t3 - t2, "round_s": t3 - t0}, shape


def med(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]} if x else None


def do_draws(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    t = trainer(sa, a)
    plain = t.pair_source(u, p)
    t.pair_source_draw(plain, 1, 1)   # (code objects loaded)
    plan = [["warm", "uniform", "draw"]]
    for name, w in weight_tables(a).items():
        src = t.pair_source(u, p, item_weight=w)
        for kind in ("draw", "hard"):
            for r in range(a.rounds + 1):
                for who in ("uniform", "form1", "form2"):
                    if who != "uniform":
                        t.set_knob("pair_weight_form", int(who[-1]))
                    t.pair_source_draw(plain if who == "uniform" else src, 1, a.seed + r, hard=a.cand if kind == "hard" else None)
                    plan.append([name, who, kind])
        src.close()
    with open(a.plan, "w") as f:
        json.dump({"items": a.items, "rows": a.rows, "factor": a.factor, "cand": a.cand, "calls": plan}, f)
    print(json.dumps({"what": "draws", "items": a.items, "rows": a.rows, "calls": len(plan)}), flush=True)
    plain.close()
    t.close()


def do_trace(a):
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace under %s, found %d" % (a.dir, len(files)))
    with open(files[0]) as f:
        disp = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)
                if "k_pair_draw" in r["Kernel_Name"] or "k_pair_hard" in r["Kernel_Name"]]
    disp.sort()
    with open(a.plan) as f:
        plan = json.load(f)
    if len(disp) != len(plan["calls"]):
        raise SystemExit("expected %d dispatches, found %d" % (len(plan["calls"]), len(disp)))
    cells = {}
    for d, (name, who, kind) in zip(disp, plan["calls"]):
        cells.setdefault((name, kind, who), []).append(d)
    for (name, kind, who), mine in cells.items():
        if name == "warm":
            continue
        names = sorted({d[2] for d in mine})
        assert len(names) == 1 and ("k_pair_hard" in names[0]) == (kind == "hard"), names
        print(json.dumps({"what": "kernel", "items": plan["items"], "rows": plan["rows"], "factor": plan["factor"], "weights": name, "pass": kind,
                          "num_cand": plan["cand"] if kind == "hard" else 0, "source": who, "kernel": names[0],
                          "kernel_ms": med([(d[1] - d[0]) * 1e-6 for d in mine[1:]])}), flush=True)


def do_rounds(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    w = weight_tables(a)[a.weights]
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a)
        t0.save_model(model)
        t0.close()
        U, A, B = trainer(sa, a, model), trainer(sa, a, model), trainer(sa, a, model)
    su, sw = U.pair_source(u, p), A.pair_source(u, p, item_weight=w)
    A.set_knob("pair_weight_form", a.form)
    out = {"uniform": [], "weighted": [], "host": []}
    host_draw = []
    for r in range(a.rounds + 1):   # one more round runs first and is not counted
        seed = a.seed + r
        order = ["uniform", "weighted", "host"]
        order = order[r % 3:] + order[:r % 3]   # the three alternate, and so does who goes first
        for who in order:
            if who == "uniform":
                res, shape = timed_round(U, lambda: U.dataset_from_pair_source(su, 1, seed))
            elif who == "weighted":
                res, shape = timed_round(A, lambda: A.dataset_from_pair_source(sw, 1, seed))
            else:
                def build():
                    t0 = time.perf_counter()
                    neg = sa.pair_negatives(a.users, a.items, u, p, 1, seed, item_weight=w)
                    host_draw.append(time.perf_counter() - t0)
                    return B.dataset_from_pairs(u, p, neg)
                res, shape = timed_round(B, build)
            if r > 0:
                out[who].append(res)
        same = all(np.array_equal(A.view(v).view(np.uint32), B.view(v).view(np.uint32)) for v in VIEWS)
        assert same, "the weighted source and the host route trained different models"
    line = {"what": "round", "config": a.config, "items": a.items, "rows": a.rows, "factor": a.factor, "weights": a.weights, "form": a.form, "shape": shape,
            "models_equal_every_round": True, "host_draw_s": med(host_draw[1:])}
    for who in out:
        line[who] = {k: med([x[k] for x in out[who]]) for k in ("round_s", "build_s", "train_s", "destroy_s")}
    line["weighted_minus_uniform_s"] = line["weighted"]["round_s"]["median"] - line["uniform"]["round_s"]["median"]
    line["weighted_exceeds_both_spreads"] = bool(line["uniform"]["round_s"]["max"] < line["weighted"]["round_s"]["min"])
    line["host_over_weighted"] = line["host"]["round_s"]["median"] / line["weighted"]["round_s"]["median"]
    line["counters"] = {who: {str(c): t.counter(c) for c in COUNTERS} for who, t in (("uniform", U), ("weighted", A), ("host", B))}
    print(json.dumps(line), flush=True)
    su.close()
    sw.close()


def planted_zipf(n, num_user, num_item, seed, rank=8):
    """tests/cases.planted_pairs with Zipf(0.7) item popularity: both items of a draw come from the popularity law (ids scattered), the
    positive is the one a planted low-rank model (with noise) prefers"""
    rng = np.random.default_rng(seed)
    law = (rng.permutation(num_item) + 1.0) ** -0.7
    law /= law.sum()
    u = rng.integers(0, num_user, n, dtype=np.int64)
    x, y = rng.choice(num_item, n, p=law), rng.choice(num_item, n, p=law)
    y = np.where(x == y, (y + 1) % num_item, y)
    pu = rng.standard_normal((num_user, rank)).astype(np.float32)
    qi = rng.standard_normal((num_item, rank)).astype(np.float32)
    first = np.einsum("nk,nk->n", pu[u], qi[x]) + 0.5 * rng.standard_normal(n) > np.einsum("nk,nk->n", pu[u], qi[y])
    return u, np.where(first, x, y)


def do_quality(a):
    import svdfeature_amd as sa
    nu, ni, n = a.users, a.items, a.rows
    u, p = planted_zipf(n, nu, ni, a.seed + 1)
    key = np.unique(u * ni + p)          # distinct (user, positive)
    rng = np.random.default_rng(a.seed + 2)
    held = rng.random(len(key)) < 0.1
    train, test = key[~held], key[held]
    tu, tp = (train // ni).astype(np.uint32), (train % ni).astype(np.uint32)
    at = rng.permutation(len(tu))
    tu, tp = tu[at], tp[at]                                # shuffled order
    users, first = np.unique(test // ni, return_index=True)   # sections: the users with held-out positives; bans: their training positives
    pos_ptr = np.append(first, len(test)).astype(np.int64)
    train_user = train // ni
    bans = (train % ni)[np.isin(train_user, users)].astype(np.uint32)
    bptr = np.concatenate([[0], np.cumsum(np.searchsorted(train_user, users, "right") - np.searchsorted(train_user, users, "left"))]).astype(np.int64)
    lists = (users.astype(np.uint32), pos_ptr, (test % ni).astype(np.uint32))
    w = sa.pair_popularity_weights(tp, ni, 0.75)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a, users=nu, items=ni)
        t0.save_model(model)
        t0.close()
        for weighted in (False, True):
            for C in (1, 8):
                t = trainer(sa, a, model, users=nu, items=ni)
                try:
                    src = t.pair_source(tu, tp, item_weight=w if weighted else None)
                except sa.SvdfError as e:
                    print(json.dumps({"what": "quality", "weighted": weighted, "num_cand": C, "refused": str(e)}), flush=True)
                    t.close()
                    continue
                curve = []
                for r in range(a.rounds):
                    ds = t.dataset_from_pair_source(src, 1, a.seed + r, hard=None if C == 1 else C)
                    t.train_dataset(ds)
                    ds.close()
                    if (r + 1) % max(1, a.rounds // 4) == 0 or r + 1 == a.rounds:
                        m = t.rank_eval(lists[0], lists[1], lists[2], bptr, bans, at=(10,), sampled=(99, a.seed + 7))
                        curve.append({"round": r + 1, "MAP": m["MAP"], "AUC": m["AUC"]})
                print(json.dumps({"what": "quality", "weighted": weighted, "num_cand": C, "users": nu, "items": ni, "train_positives": len(tu), "held_out": len(test),
                                  "sections": len(users), "factor": a.factor, "learning_rate": a.learning_rate, "rounds": a.rounds, "curve": curve,
                                  "counters": {str(c): t.counter(c) for c in COUNTERS}}), flush=True)
                src.close()
                t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["draws", "trace", "rounds", "quality"])
    ap.add_argument("dir", nargs="?", help="trace: the profiler's output directory")
    ap.add_argument("--plan", default="pair_weight_plan.json", help="draws writes the order of its calls here, trace reads it")
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--factor", type=int, default=128)
    ap.add_argument("--cand", type=int, default=8, help="draws: num_cand of the hard pass")
    ap.add_argument("--weights", default="zipf", choices=["zipf", "equal"], help="rounds: the weight table")
    ap.add_argument("--form", type=int, default=0, help="rounds: knob pair_weight_form")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds or calls per cell (one more runs first)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learning-rate", type=float, default=0.005)
    ap.add_argument("--config", default="exact", choices=["exact", "minibatch"])
    a = ap.parse_args()
    {"draws": do_draws, "trace": do_trace, "rounds": do_rounds, "quality": do_quality}[a.what](a)


if __name__ == "__main__":
    main()

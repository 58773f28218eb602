#!/usr/bin/env python3
"""Shuffled passes of a pair source on one GPU (results in profiles/r38_pair_order.md).  Each measurement is a process
of its own printing JSON lines:

    python tools/pair_order.py rounds  [--config exact|minibatch]
        (a) a shuffled round (build + train + synchronize + destroy) of dataset_from_pair_source(src, 1, seed, shuffle=s) against the two routes
        to the same pass WITHOUT the order on the device, on three trainers started from one model file, alternating round by round:
        `source`  a host permutation, a new pair_source of the permuted rows, a plain pass, the source destroyed;
        `host`    a host permutation, pair_negatives on the permuted rows, dataset_from_pairs.
        The host permutation is timed as numpy's Generator.permutation(n) plus the two gathers; the gathers use pair_order(n, s), computed
        outside the clock, so that the three trainers train the same pass: their models are asserted equal bit for bit after every round.
    python tools/pair_order.py cost    [--config exact|minibatch]
        (b) the shuffled round against the unshuffled pass of the same build, alternating on one trainer and one source shuffled once
    python tools/pair_order.py grouped
        (c) a user-grouped source: shuffled rounds (the HBM route) against unshuffled ones (user-run units through the fallback), counters 44 / 45
        recorded.  Different passes; reported as such.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pair_order.py draws
    python tools/pair_order.py trace DIR
        (d) k_pair_order alone: `draws` only calls pair_source_draw(shuffle=) --rounds + 1 times under the profiler; `trace` reads the dispatches
    python tools/pair_order.py quality [--learning-rate 0.02]
        (e) the planted set of tools/pair_hard.py quality, --rounds rounds: a fixed order (shuffled once) against shuffle=round, for the plain
        pass and hard=8, by rank_eval(sampled=) on --data-seeds data seeds.  Reported, not asserted.
    python tools/pair_order.py report FILE.jsonl
        the tables of profiles/r38_pair_order.md from the lines above, on standard output

The source is section 6ac's shape: --users x --items, --rows positives."""
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

COUNTERS = (44, 45, 46, 47, 48)
VIEWS = ("W_user", "W_item", "i_bias")


def rows(a, grouped=False):
    """--rows positives in shuffled order (tools/pair_source.py's source), or the same rows grouped by user"""
    rng = np.random.default_rng(a.seed)
    u = rng.integers(0, a.users, a.rows).astype(np.uint32)
    p = ((u.astype(np.int64) * 7919 + rng.integers(0, a.items // 2, a.rows)) % a.items).astype(np.uint32)
    if grouped:
        at = np.argsort(u, kind="stable")
        u, p = u[at], p[at]
    return u, p


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


def timed_round(t, build, after=None):
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
    if after:
        after()
    t.synchronize()
    t3 = time.perf_counter()
    return {"build_s": t1 - t0, "train_s": t2 - t1, "destroy_s": t3 - t2, "round_s": t3 - t0}, shape


def med(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]} if x else None


def summary(out, keys=("round_s", "build_s", "train_s", "destroy_s")):
    return {who: {k: med([x[k] for x in res]) for k in keys} for who, res in out.items()}


def counters(t):
    return {str(c): t.counter(c) for c in COUNTERS}


def models_equal(ts):
    first = [ts[0].view(v).view(np.uint32) for v in VIEWS]
    return all(np.array_equal(x, t.view(v).view(np.uint32)) for t in ts[1:] for x, v in zip(first, VIEWS))


def do_rounds(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    n = len(u)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a)
        t0.save_model(model)
        t0.close()
        T = {who: trainer(sa, a, model) for who in ("shuffled", "source", "host")}
    src = T["shuffled"].pair_source(u, p)
    out = {who: [] for who in T}
    parts = {"permute_s": [], "create_s": [], "negatives_s": []}
    rng = np.random.default_rng(a.seed + 5)
    equal = []
    for r in range(a.rounds + 1):   # one more round runs first and is not counted
        seed, s = a.seed + r, a.seed + 100 + r
        sigma = sa.pair_order(n, s).astype(np.int64)   # outside every clock: what makes the three passes one pass
        who_order = ("shuffled", "source", "host") if r % 2 == 0 else ("host", "source", "shuffled")
        shapes = {}
        for who in who_order:
            t = T[who]
            if who == "shuffled":
                res, shapes[who] = timed_round(t, lambda: t.dataset_from_pair_source(src, 1, seed, shuffle=s))
                res["permute_s"] = 0.0
            else:
                t.synchronize()
                c0 = time.perf_counter()
                rng.permutation(n)                      # the order a caller without the rule would draw
                pu, pp = u[sigma], p[sigma]             # ... and the gathers, with the order that makes the passes comparable
                c1 = time.perf_counter()
                if who == "source":
                    s2 = t.pair_source(pu, pp)
                    c2 = time.perf_counter()
                    res, shapes[who] = timed_round(t, lambda: t.dataset_from_pair_source(s2, 1, seed), after=s2.close)
                    if r > 0:
                        parts["create_s"].append(c2 - c1)
                else:
                    neg = sa.pair_negatives(a.users, a.items, pu, pp, 1, seed)
                    c2 = time.perf_counter()
                    res, shapes[who] = timed_round(t, lambda: t.dataset_from_pairs(pu, pp, neg))
                    if r > 0:
                        parts["negatives_s"].append(c2 - c1)
                res["permute_s"] = c1 - c0
                res["round_s"] += c2 - c0
                res["build_s"] += c2 - c0
                if r > 0:
                    parts["permute_s"].append(c1 - c0)
            if r > 0:
                out[who].append(res)
        assert shapes["shuffled"] == shapes["source"] == shapes["host"], shapes
        equal.append(models_equal(list(T.values())))
        assert equal[-1], "the models of the three routes differ after round %d" % r
    line = {"what": "rounds", "config": a.config, "factor": a.factor, "rows": n, "shape": shapes["shuffled"], "models_equal_after_every_round": all(equal),
            "rounds_compared": len(equal), **summary(out), "parts": {k: med(v) for k, v in parts.items()},
            "counters": {who: counters(t) for who, t in T.items()}}
    for who in ("source", "host"):
        line["%s_over_shuffled" % who] = line[who]["round_s"]["median"] / line["shuffled"]["round_s"]["median"]
        line["%s_exceeds_both_spreads" % who] = bool(line["shuffled"]["round_s"]["max"] < line[who]["round_s"]["min"])
    print(json.dumps(line), flush=True)
    src.close()
    for t in T.values():
        t.close()


def alternate(a, t, src, what, plain_first_name="unshuffled"):
    out = {plain_first_name: [], "shuffled": []}
    shapes = {}
    for r in range(a.rounds + 1):
        seed, s = a.seed + r, a.seed + 100 + r
        order = (plain_first_name, "shuffled") if r % 2 == 0 else ("shuffled", plain_first_name)
        for who in order:
            res, shapes[who] = timed_round(t, (lambda: t.dataset_from_pair_source(src, 1, seed)) if who != "shuffled" else
                                           (lambda: t.dataset_from_pair_source(src, 1, seed, shuffle=s)))
            if r > 0:
                out[who].append(res)
    line = {"what": what, "config": a.config, "factor": a.factor, "rows": a.rows, "shapes": shapes, **summary(out), "counters": counters(t)}
    pl, sh = line[plain_first_name]["round_s"], line["shuffled"]["round_s"]
    line["shuffled_minus_%s_s" % plain_first_name] = sh["median"] - pl["median"]
    line["exceeds_both_spreads"] = bool(pl["max"] < sh["min"] or sh["max"] < pl["min"])
    print(json.dumps(line), flush=True)


def do_cost(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    t = trainer(sa, a)
    src = t.pair_source(u, p)
    alternate(a, t, src, "cost")
    src.close()
    t.close()


def do_grouped(a):
    import svdfeature_amd as sa
    u, p = rows(a, grouped=True)
    t = trainer(sa, a)
    src = t.pair_source(u, p)
    alternate(a, t, src, "grouped")
    src.close()
    t.close()


def do_draws(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    t = trainer(sa, a)
    src = t.pair_source(u, p)
    t.pair_source_draw(src, 1, 1)   # (code objects loaded)
    for r in range(a.rounds + 1):
        t.pair_source_draw(src, 1, a.seed + r, shuffle=a.seed + 100 + r)
    print(json.dumps({"what": "draws", "rows": a.rows, "calls": a.rounds + 1}), flush=True)
    src.close()
    t.close()


def do_trace(a):
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace under %s, found %d" % (a.dir, len(files)))
    with open(files[0]) as f:
        disp = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    for name, calls in (("k_pair_order", a.rounds + 1), ("k_pair_draw", a.rounds + 2)):
        mine = sorted(d for d in disp if name in d[2])
        if len(mine) != calls:
            raise SystemExit("expected %d dispatches of %s, found %d" % (calls, name, len(mine)))
        mine = mine[-a.rounds:]   # the shuffled calls, the first of them not counted
        t = med([(d[1] - d[0]) * 1e-9 for d in mine])
        moved = a.rows * 16       # two gathers and two stores of 4 bytes per row
        print(json.dumps({"what": "kernel", "kernel": name, "rows": a.rows, "kernel_s": t, "bytes_if_order": moved,
                          "tb_per_s_if_order": moved / t["median"] * 1e-12}), flush=True)


def do_quality(a):
    import svdfeature_amd as sa
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    nu, ni, n = a.users, a.items, a.rows
    for data_seed in range(a.seed, a.seed + a.data_seeds):
        u, p, _ = cases.planted_pairs(n, nu, ni, seed=data_seed + 1)
        key = np.unique(u.astype(np.int64) * ni + p)          # distinct (user, positive)
        rng = np.random.default_rng(data_seed + 2)
        held = rng.random(len(key)) < 0.1
        train, test = key[~held], key[held]
        tu, tp = (train // ni).astype(np.uint32), (train % ni).astype(np.uint32)
        at = rng.permutation(len(tu))
        tu, tp = tu[at], tp[at]                                # shuffled once
        users, first = np.unique(test // ni, return_index=True)
        pos_ptr = np.append(first, len(test)).astype(np.int64)
        train_user = train // ni
        bans = (train % ni)[np.isin(train_user, users)].astype(np.uint32)
        bptr = np.concatenate([[0], np.cumsum(np.searchsorted(train_user, users, "right") - np.searchsorted(train_user, users, "left"))]).astype(np.int64)
        lists = (users.astype(np.uint32), pos_ptr, (test % ni).astype(np.uint32))
        with tempfile.TemporaryDirectory() as tmp:
            model = os.path.join(tmp, "model")
            t0 = trainer(sa, a, users=nu, items=ni)
            t0.save_model(model)
            t0.close()
            for C in (None, 8):
                for order in ("fixed", "shuffled"):
                    t = trainer(sa, a, model, users=nu, items=ni)
                    src = t.pair_source(tu, tp)
                    curve = []
                    for r in range(a.rounds):
                        ds = t.dataset_from_pair_source(src, 1, data_seed + r, hard=C, shuffle=None if order == "fixed" else r)
                        t.train_dataset(ds)
                        ds.close()
                        if (r + 1) % max(1, a.rounds // 4) == 0 or r + 1 == a.rounds:
                            m = t.rank_eval(lists[0], lists[1], lists[2], bptr, bans, at=(10,), sampled=(99, data_seed + 7))
                            curve.append({"round": r + 1, "MAP": m["MAP"], "AUC": m["AUC"]})
                    print(json.dumps({"what": "quality", "data_seed": data_seed, "hard": C or 1, "order": order, "users": nu, "items": ni,
                                      "train_positives": len(tu), "held_out": len(test), "factor": a.factor, "learning_rate": a.learning_rate,
                                      "rounds": a.rounds, "curve": curve, "counters": counters(t)}), flush=True)
                    src.close()
                    t.close()


def cell(m, scale=1.0, fmt="%.4f"):
    return (fmt + " (" + fmt + " .. " + fmt + ")") % (m["median"] * scale, m["min"] * scale, m["max"] * scale)


def do_report(a):
    lines = [json.loads(x) for x in open(a.dir) if x.startswith("{")]
    print("## (a) a shuffled round against the two routes without the order on the device (seconds)\n")
    print("| step | shuffled round | new source per round | ratio | host negatives + dataset_from_pairs | ratio | models equal |\n|---|---|---|---|---|---|---|")
    for x in (x for x in lines if x["what"] == "rounds"):
        print("| %s | %s | %s | %.1f x | %s | %.1f x | %s, %d rounds |" % (x["config"], cell(x["shuffled"]["round_s"]), cell(x["source"]["round_s"]), x["source_over_shuffled"],
                                                                    cell(x["host"]["round_s"]), x["host_over_shuffled"], x["models_equal_after_every_round"], x["rounds_compared"]))
    print("\n## (b), (c) shuffled against unshuffled rounds of the same build (seconds)\n")
    print("| source | step | unshuffled round | shuffled round | shuffled - unshuffled | outside both spreads | shuffled build | unshuffled build | counters 44 / 45 / 48 |\n|---|---|---|---|---|---|---|---|---|")
    for x in (x for x in lines if x["what"] in ("cost", "grouped")):
        print("| %s | %s | %s | %s | %+.1f ms | %s | %.4f | %.4f | %d / %d / %d |" % (
            "shuffled once" if x["what"] == "cost" else "user-grouped", x["config"], cell(x["unshuffled"]["round_s"]), cell(x["shuffled"]["round_s"]),
            1e3 * x["shuffled_minus_unshuffled_s"], x["exceeds_both_spreads"], x["shuffled"]["build_s"]["median"], x["unshuffled"]["build_s"]["median"],
            x["counters"]["44"], x["counters"]["45"], x["counters"]["48"]))
    print("\n## (d) the kernels alone (milliseconds)\n\n| kernel | time | TB/s over 16 B per row |\n|---|---|---|")
    for x in (x for x in lines if x["what"] == "kernel"):
        print("| %s | %s | %s |" % (x["kernel"], cell(x["kernel_s"], 1e3, "%.3f"), "%.2f" % x["tb_per_s_if_order"] if x["kernel"] == "k_pair_order" else "--"))
    print("\n## (e) planted set: MAP / AUC after the last round\n\n| data seed | hard | fixed order | shuffle = round |\n|---|---|---|---|")
    q = [x for x in lines if x["what"] == "quality"]
    for seed in sorted({x["data_seed"] for x in q}):
        for C in (1, 8):
            got = {x["order"]: x["curve"][-1] for x in q if x["data_seed"] == seed and x["hard"] == C}
            if len(got) == 2:
                print("| %d | %d | %.4f / %.4f | %.4f / %.4f |" % (seed, C, got["fixed"]["MAP"], got["fixed"]["AUC"], got["shuffled"]["MAP"], got["shuffled"]["AUC"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rounds", "cost", "grouped", "draws", "trace", "quality", "report"])
    ap.add_argument("dir", nargs="?", help="trace: the profiler's output directory; report: the file of JSON lines")
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--factor", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds (one more runs first)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--data-seeds", type=int, default=3)
    ap.add_argument("--learning-rate", type=float, default=0.005)
    ap.add_argument("--config", default="exact", choices=["exact", "minibatch"])
    a = ap.parse_args()
    {"rounds": do_rounds, "cost": do_cost, "grouped": do_grouped, "draws": do_draws, "trace": do_trace, "quality": do_quality, "report": do_report}[a.what](a)


if __name__ == "__main__":
    main()

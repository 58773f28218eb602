#!/usr/bin/env python3
"""Hard negatives for pair-source passes on one GPU (results in profiles/r34_pair_hard.md).  Four measurements, each a
process of its own printing JSON lines:

    python tools/pair_hard.py rounds  [--factor 128] [--config exact|minibatch]
        round time (build + train + synchronize + destroy) of dataset_from_pair_source(src, 1, seed, hard=C) for C in --cands, alternating
        round by round with the plain pass of the same build on the same trainer and source; medians of --rounds with min .. max
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/pair_hard.py draws [--factor 128]
    python tools/pair_hard.py trace DIR [--factor 128]
        k_pair_hard's own time: `draws` only calls pair_source_draw(hard=C) -- form 1, then form 2, each C of --cands --rounds times after one
        uncounted call -- under the profiler; `trace` reads the dispatches of DIR's kernel trace in that order and prints per (form, C) the
        median time and the rate at which the kernel moves its n * C * pitch * 4 bytes of item rows
    python tools/pair_hard.py parent  [--rows 1000000]
        the same negatives through the only route before the hard pass -- pair_source_draw(src, C) to the host, rank_topn(users, 1,
        candidates=) with one section per row, dataset_from_pairs -- alternating with the hard pass; the negatives are asserted equal on
        every row whose two best candidates do not tie
    python tools/pair_hard.py quality
        a planted implicit-feedback set (tests/cases.planted_pairs scaled up, a tenth of the positives held out): MAP and AUC of
        rank_eval(..., sampled=(99, seed)) after --rounds rounds with hard in (1, 8) from the same start.  Reported, not asserted.

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

C_HBM, C_FALLBACK, C_HARD = 44, 45, 46


def rows(a):
    """--rows positives in shuffled order; every user draws from its own half of the items (tools/pair_source.py's source)"""
    rng = np.random.default_rng(a.seed)
    u = rng.integers(0, a.users, a.rows).astype(np.uint32)
    p = ((u.astype(np.int64) * 7919 + rng.integers(0, a.items // 2, a.rows)) % a.items).astype(np.uint32)
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


def timed_round(t, build):
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


def med(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]} if x else None


def cands(a):
    return [int(c) for c in a.cands.split(",")]


def do_rounds(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    t = trainer(sa, a)
    src = t.pair_source(u, p)
    t.set_knob("pair_hard_form", a.form)
    for C in cands(a):
        out = {"plain": [], "hard": []}
        for r in range(a.rounds + 1):   # one more round runs first and is not counted
            seed = a.seed + 1000 * C + r
            order = ("plain", "hard") if r % 2 == 0 else ("hard", "plain")   # the two alternate, and so does who goes first
            for who in order:
                res, shape = timed_round(t, (lambda: t.dataset_from_pair_source(src, 1, seed)) if who == "plain" else
                                         (lambda: t.dataset_from_pair_source(src, 1, seed, hard=C)))
                if r > 0:
                    out[who].append(res)
        line = {"what": "round", "config": a.config, "factor": a.factor, "rows": a.rows, "num_cand": C, "form": a.form, "shape": shape}
        for who in ("plain", "hard"):
            line[who] = {k: med([x[k] for x in out[who]]) for k in ("round_s", "build_s", "train_s", "destroy_s")}
        pl, hd = line["plain"]["round_s"], line["hard"]["round_s"]
        line["hard_minus_plain_s"] = hd["median"] - pl["median"]
        line["exceeds_both_spreads"] = bool(pl["max"] < hd["min"])
        print(json.dumps(line), flush=True)
    print(json.dumps({"what": "counters", "config": a.config, "factor": a.factor, **{str(c): t.counter(c) for c in (C_HBM, C_FALLBACK, C_HARD)}}), flush=True)
    src.close()
    t.close()


def do_draws(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    t = trainer(sa, a)
    src = t.pair_source(u, p)
    t.pair_source_draw(src, 1, 1)   # (code objects loaded)
    for form in (1, 2):
        t.set_knob("pair_hard_form", form)
        for C in cands(a):
            for r in range(a.rounds + 1):
                t.pair_source_draw(src, 1, a.seed + r, hard=C)
    print(json.dumps({"what": "draws", "factor": a.factor, "rows": a.rows, "cands": cands(a), "calls_per_cell": a.rounds + 1}), flush=True)
    src.close()
    t.close()


def do_trace(a):
    files = glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit("expected one kernel trace under %s, found %d" % (a.dir, len(files)))
    with open(files[0]) as f:
        disp = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f) if "k_pair_hard" in r["Kernel_Name"]]
    disp.sort()
    per = a.rounds + 1
    if len(disp) != 2 * len(cands(a)) * per:
        raise SystemExit("expected %d dispatches of k_pair_hard, found %d" % (2 * len(cands(a)) * per, len(disp)))
    pitch = a.pitch or ((a.factor + 3) // 4) * 4
    at = 0
    for form in (1, 2):
        for C in cands(a):
            mine = disp[at:at + per]
            at += per
            names = sorted({d[2] for d in mine})
            t = med([(d[1] - d[0]) * 1e-9 for d in mine[1:]])
            gathered = a.rows * C * pitch * 4
            print(json.dumps({"what": "kernel", "factor": a.factor, "pitch": pitch, "rows": a.rows, "form": form, "num_cand": C, "kernel": names, "kernel_s": t,
                              "item_row_bytes": gathered, "item_row_tb_per_s": gathered / t["median"] * 1e-12}), flush=True)


def do_parent(a):
    import svdfeature_amd as sa
    u, p = rows(a)
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a)
        t0.save_model(model)
        t0.close()
        A, B = trainer(sa, a, model), trainer(sa, a, model)
    sa_, sb = A.pair_source(u, p), B.pair_source(u, p)
    n = len(u)
    for C in cands(a):
        ptr = C * np.arange(n + 1, dtype=np.int64)
        out = {"hard": [], "parent": []}
        for r in range(a.rounds + 1):
            seed = a.seed + 1000 * C + r
            # the check, untimed, on the model as it stands: equal wherever the two best candidates do not tie
            cand = B.pair_source_draw(sb, C, seed)
            items, scores, count, nan = B.rank_topn(u, min(2, C), candidates=(ptr, cand))
            got = A.pair_source_draw(sa_, 1, seed, hard=C)
            tied = (scores[:, 0] == scores[:, 1]) & (items[:, 0] != items[:, 1]) if C > 1 else np.zeros(n, bool)
            assert not nan.any() and np.array_equal(got[~tied], items[~tied, 0].astype(np.uint32)), "the two routes disagree on an untied row"
            order = ("hard", "parent") if r % 2 == 0 else ("parent", "hard")
            for who in order:
                if who == "hard":
                    res, shape = timed_round(A, lambda: A.dataset_from_pair_source(sa_, 1, seed, hard=C))
                else:
                    def build():
                        c = B.pair_source_draw(sb, C, seed)
                        best = B.rank_topn(u, 1, candidates=(ptr, c))[0][:, 0].astype(np.uint32)
                        return B.dataset_from_pairs(u, p, best)
                    res, shape_b = timed_round(B, build)
                if r > 0:
                    out[who].append(res)
            assert shape == shape_b, (shape, shape_b)
            same = all(np.array_equal(A.view(v).view(np.uint32), B.view(v).view(np.uint32)) for v in ("W_user", "W_item", "i_bias"))
            assert same or tied.any(), "the models of the two routes differ without a tie"
        line = {"what": "parent", "config": a.config, "factor": a.factor, "rows": n, "num_cand": C, "tied_rows_last_round": int(tied.sum()), "models_equal_last_round": bool(same)}
        for who in ("hard", "parent"):
            line[who] = {k: med([x[k] for x in out[who]]) for k in ("round_s", "build_s", "train_s")}
        line["ratio_of_medians"] = line["parent"]["round_s"]["median"] / line["hard"]["round_s"]["median"]
        line["exceeds_both_spreads"] = bool(line["hard"]["round_s"]["max"] < line["parent"]["round_s"]["min"])
        print(json.dumps(line), flush=True)
    sa_.close()
    sb.close()


def do_quality(a):
    import svdfeature_amd as sa
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cases
    nu, ni, n = a.users, a.items, a.rows
    u, p, _ = cases.planted_pairs(n, nu, ni, seed=a.seed + 1)
    key = np.unique(u.astype(np.int64) * ni + p)          # distinct (user, positive)
    rng = np.random.default_rng(a.seed + 2)
    held = rng.random(len(key)) < 0.1
    train, test = key[~held], key[held]
    tu, tp = (train // ni).astype(np.uint32), (train % ni).astype(np.uint32)
    at = rng.permutation(len(tu))
    tu, tp = tu[at], tp[at]                                # shuffled order
    users, first = np.unique(test // ni, return_index=True)   # sections: the users with held-out positives; bans: their training positives
    pos_ptr = np.append(first, len(test)).astype(np.int64)
    train_user = train // ni                                  # sorted, like users: the bans of the sections are the masked items, in order
    bans = (train % ni)[np.isin(train_user, users)].astype(np.uint32)
    bptr = np.concatenate([[0], np.cumsum(np.searchsorted(train_user, users, "right") - np.searchsorted(train_user, users, "left"))]).astype(np.int64)
    lists = (users.astype(np.uint32), pos_ptr, (test % ni).astype(np.uint32))
    with tempfile.TemporaryDirectory() as tmp:
        model = os.path.join(tmp, "model")
        t0 = trainer(sa, a, users=nu, items=ni)
        t0.save_model(model)
        t0.close()
        for C in (1, 8):
            t = trainer(sa, a, model, users=nu, items=ni)
            src = t.pair_source(tu, tp)
            curve = []
            for r in range(a.rounds):
                ds = t.dataset_from_pair_source(src, 1, a.seed + r, hard=C)
                t.train_dataset(ds)
                ds.close()
                if (r + 1) % max(1, a.rounds // 5) == 0 or r + 1 == a.rounds:
                    m = t.rank_eval(lists[0], lists[1], lists[2], bptr, bans, at=(10,), sampled=(99, a.seed + 7))
                    curve.append({"round": r + 1, "MAP": m["MAP"], "AUC": m["AUC"]})
            print(json.dumps({"what": "quality", "num_cand": C, "users": nu, "items": ni, "train_positives": len(tu), "held_out": len(test), "sections": len(users),
                              "factor": a.factor, "learning_rate": a.learning_rate, "rounds": a.rounds, "curve": curve}), flush=True)
            src.close()
            t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rounds", "draws", "trace", "parent", "quality"])
    ap.add_argument("dir", nargs="?", help="trace: the profiler's output directory")
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--factor", type=int, default=128)
    ap.add_argument("--pitch", type=int, default=0, help="trace: floats between two rows of the model (default: num_factor rounded up to 4)")
    ap.add_argument("--cands", default="2,4,8,16")
    ap.add_argument("--form", type=int, default=0, help="rounds: knob pair_hard_form")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per cell (one more runs first)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--learning-rate", type=float, default=0.005)
    ap.add_argument("--config", default="exact", choices=["exact", "minibatch"])
    a = ap.parse_args()
    {"rounds": do_rounds, "draws": do_draws, "trace": do_trace, "parent": do_parent, "quality": do_quality}[a.what](a)


if __name__ == "__main__":
    main()

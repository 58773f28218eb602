#!/usr/bin/env python3
"""Round loop over a candidate file (input_type = 2) on one GPU: time per round of svdf_dataset_from_rank_buffer_file + svdf_train_dataset +
synchronize + destroy under `amd:step` = (none) / minibatch / auto, and held-out pair accuracy after equal rounds against the exact pass of the
same build (results in profiles/r23_rank_window.md).

The file has the shape of demo/pairwiseRank at the scale of benchlib/orders.py's generator case divided by ten: one block per user, `--rows`
candidate rows (one user entry, one item entry, values 1, items distinct inside a block), labels from a planted preference model (item biases + rank 8);
rank_sample_num = --per-user pairs are drawn per block, so one pass draws users x per-user pairs in the generator's order.

    python tools/rank_window.py                          # this build: timing at 20 M pairs per pass, accuracy at 4 M on three data seeds
    python tools/rank_window.py --other-lib PATH         # the same, alternating with another build of libsvdfeature_amd.so (the parent commit's)

Every configuration runs in a process of its own (--child); builds alternate inside one session."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def planted(users, items, seed):
    """score(u, i) = b_i + <p_u, q_i> / 2 sqrt(8): user factors, item factors, item biases"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((users, 8)).astype(np.float32), (rng.standard_normal((items, 8)) / (2.0 * np.sqrt(8.0))).astype(np.float32),
            (0.5 * rng.standard_normal(items)).astype(np.float32))


def write_candidates(path, users, rows, items, seed):
    """one block per user, users in random order; a block's items are one random set of `rows` distinct offsets rotated by a per-block base"""
    rng = np.random.default_rng(seed + 1)
    pu, qi, bi = planted(users, items, seed)
    rec = np.dtype([("nfb", "<i4"), ("num_row", "<i4"), ("num_val", "<i4"), ("row_ptr", "<i4", (3 * rows + 1,)),
                    ("label", "<f4", (rows,)), ("index", "<u4", (2 * rows,)), ("value", "<f4", (2 * rows,))])
    a = np.zeros(users, rec)
    a["num_row"] = rows
    a["num_val"] = 2 * rows
    rp = np.zeros(3 * rows + 1, np.int32)
    rp[1::3] = 2 * np.arange(rows)
    rp[2::3] = 2 * np.arange(rows) + 1
    rp[3::3] = 2 * np.arange(rows) + 2
    a["row_ptr"] = rp
    uid = rng.permutation(users).astype(np.uint32)
    offs = rng.choice(items, size=rows, replace=False)
    it = ((rng.integers(0, items, users)[:, None] + offs[None, :]) % items).astype(np.uint32)
    score = bi[it] + np.einsum("uk,urk->ur", pu[uid], qi[it]) + 0.35 * rng.standard_normal((users, rows)).astype(np.float32)
    a["label"] = (score > 0).astype(np.float32)
    a["index"][:, 0::2] = uid[:, None]
    a["index"][:, 1::2] = it
    a["value"] = 1.0
    with open(path, "wb") as f:
        np.array([users, 0, rows, 2 * rows], np.int32).tofile(f)
        a.tofile(f)


def held_out(users, items, seed, n=200_000):
    rng = np.random.default_rng(seed + 2)
    pu, qi, bi = planted(users, items, seed)
    u = rng.integers(0, users, n)
    x = rng.integers(0, items, n)
    y = (x + 1 + rng.integers(0, items - 1, n)) % items
    first = bi[x] + np.einsum("nk,nk->n", pu[u], qi[x]) > bi[y] + np.einsum("nk,nk->n", pu[u], qi[y])
    return u, np.where(first, x, y), np.where(first, y, x)


def child(a):
    import svdfeature_amd as sa
    if a.lib:
        sa.LIB_PATH = a.lib
    t = sa.Trainer(1, 3)
    t.seed(10)
    conf = [("num_user", a.users), ("num_item", a.items), ("num_global", 0), ("num_factor", a.factor), ("num_ufeedback", 0), ("learning_rate", 0.005),
            ("wd_user", 0.004), ("wd_item", 0.004), ("no_user_bias", 1), ("ui_init_sigma", 0.1), ("rank_sample_num", a.per_user), ("rank_sample_max", a.per_user)]
    if a.step != "none":
        conf.append(("amd:step", a.step))
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    out = {"step": a.step, "lib": a.lib or "this", "build_s": [], "train_s": [], "round_s": [], "kinds": [], "windows": [], "pairs": 0}
    for r in range(a.rounds):
        t.set_round(r)
        t.synchronize()
        t0 = time.perf_counter()
        ds = t.dataset_from_rank_buffer_file(a.src)
        t.synchronize()
        t1 = time.perf_counter()
        t.train_dataset(ds)
        t.finish_round()
        t.synchronize()
        t2 = time.perf_counter()
        out["kinds"].append([ds.kind, ds.info(8)])
        out["windows"].append(ds.num_batches)
        out["pairs"] = ds.num_row
        ds.close()
        t3 = time.perf_counter()
        out["build_s"].append(t1 - t0)
        out["train_s"].append(t2 - t1)
        out["round_s"].append(t3 - t0)
    out["counters"] = {str(c): t.counter(c) for c in (7, 16, 37)}
    u, p, q = held_out(a.users, a.items, a.seed)
    wu, wi, bi = t.view("W_user"), t.view("W_item"), t.view("i_bias")
    d = np.einsum("nk,nk->n", wu[u], wi[p] - wi[q]) + bi[p] - bi[q]
    out["finite"] = bool(np.isfinite(wu).all() and np.isfinite(wi).all())
    out["accuracy"] = float(np.mean(d > 0))
    t.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(a, src, users, seed, step, lib, rounds):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--src", src, "--users", str(users), "--items", str(a.items), "--factor", str(a.factor),
           "--per-user", str(a.per_user), "--rounds", str(rounds), "--seed", str(seed), "--step", step]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, SVDF_PROFILE="1"), timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit("child failed (%d): %s\n%s" % (p.returncode, " ".join(cmd), p.stderr[-2000:]))
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    m = re.search(r"rank-buffer route: (\d+) passes .*draw ([0-9.]+)s, item counts \+ window rule ([0-9.]+)s, window build ([0-9.]+)s", p.stderr)
    if m:
        n = int(m.group(1))
        res["phase_mean_s"] = {"passes": n, "draw": float(m.group(2)) / n, "rule": float(m.group(3)) / n, "window_build": float(m.group(4)) / n}
    return res


def med(x):
    x = sorted(x)
    return {"median": x[len(x) // 2], "min": x[0], "max": x[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--acc-users", type=int, default=20_000)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--per-user", type=int, default=200)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--factor", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds (one more runs first: file load, first-pass decision of auto)")
    ap.add_argument("--acc-rounds", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--other-lib", default="")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--src")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--step", default="none")
    ap.add_argument("--lib", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "cand.buffer")
        write_candidates(src, a.users, a.rows, a.items, 0)
        runs = [("", "minibatch"), ("", "auto")]
        if a.other_lib:
            runs = [(a.other_lib, "auto"), ("", "minibatch"), (a.other_lib, "minibatch"), ("", "auto")]
        for lib, step in ([] if a.skip_timing else runs):
            r = run_child(a, src, a.users, 0, step, lib, a.rounds + 1)
            line = {"what": "timing", "build": "other" if lib else "this", "step": step, "pairs_per_pass": r["pairs"], "kinds": r["kinds"][-1], "windows": r["windows"][-1],
                    "counters": r["counters"], "round_s": med(r["round_s"][1:]), "build_s": med(r["build_s"][1:]), "train_s": med(r["train_s"][1:]),
                    "first_round_s": r["round_s"][0], "phase_mean_s": r.get("phase_mean_s")}
            line["pairs_per_s"] = r["pairs"] / line["round_s"]["median"]
            print(json.dumps(line), flush=True)
        os.unlink(src)
        for seed in range(1, a.seeds + 1):
            write_candidates(src, a.acc_users, a.rows, a.items, seed)
            acc = {}
            for step in ("none", "minibatch", "auto"):
                r = run_child(a, src, a.acc_users, seed, step, "", a.acc_rounds)
                acc[step] = r["accuracy"]
                assert r["finite"], (seed, step)
            print(json.dumps({"what": "accuracy", "data_seed": seed, "pairs_per_pass": r["pairs"], "rounds": a.acc_rounds, "exact": acc["none"],
                              "minibatch_minus_exact": acc["minibatch"] - acc["none"], "auto_minus_exact": acc["auto"] - acc["none"], "auto_kinds": r["kinds"]}), flush=True)
            os.unlink(src)


if __name__ == "__main__":
    main()

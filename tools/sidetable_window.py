#!/usr/bin/env python3
"""The SURVEY 8(d2) side-feature variant expressed through feature_user / feature_item side tables, on one MI355X, exact pass against the
window step (`amd:step = minibatch`).  Rows: 4 distinct global ids out of 10 K (values U(0,1)), the user and the track.
The tables carry the attributes: every user has one of 64 age buckets and one of 16 regions (user ids after the 1 M users, at or above
amd:shared_user_from = 1 M); every track (100 K) has its album (of 10 K), its artist (of 2 K, the album's) and one of 256 genres (item ids
after the tracks).  k = 64.

  exact      the default exact level-scheduled pass (each region row is a dependency chain of n / 16 updates)
  window     amd:step = minibatch + amd:shared_user_from = 1 M at the default rule (knob window_per_target_child: the updates a child row meets
             per window on average) and at the window_per_target_child values listed in --schemes

Throughput of the first seed (ms and inst/s per pass over passes 2 .. 3, windows per pass, data-set build time), then |dRMSE| of each window
scheme against the exact pass after the passes, on a held-out set, for every data seed.  --n rows per pass.
usage: python tools/sidetable_window.py --n 20000000 --test 1000000 --seeds 1,2,3 --out profiles/r08_sidetable_window.md"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdfeature_amd as sa
from svdfeature_amd import CSRData

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--test", type=int, default=200_000)
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--factor", type=int, default=64)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--seeds", default="1,2,3")
ap.add_argument("--out", default="")
ap.add_argument("--schemes", default="exact,window", help="exact, window (the default rule) and window_per_target_child values, e.g. exact,window,8")
ap.add_argument("--no-drmse", action="store_true", help="throughput only (no held-out comparison needs every scheme of a seed)")
a = ap.parse_args()
NG, G = 4, 10000
NB, NR = 64, 16                  # age buckets, regions
NAL, NAR, NGE = 10000, 2000, 256  # albums, artists, genres
NU, NI = a.users + NB + NR, a.items + NAL + NAR + NGE


def tables(rng, tmp):
    """the user and item side tables of one data seed, as files"""
    fu, fi = os.path.join(tmp, "feature_user.txt"), os.path.join(tmp, "feature_item.txt")
    bucket = a.users + rng.integers(0, NB, a.users)
    region = a.users + NB + rng.integers(0, NR, a.users)
    with open(fu, "w") as f:
        f.write("".join("2 %d:1 %d:1\n" % (b, r) for b, r in zip(bucket.tolist(), region.tolist())))
    album = rng.integers(0, NAL, a.items)
    artist = a.items + NAL + album % NAR
    genre = a.items + NAL + NAR + rng.integers(0, NGE, a.items)
    with open(fi, "w") as f:
        f.write("".join("3 %d:1 %d:1 %d:1\n" % (al, ar, g) for al, ar, g in zip((a.items + album).tolist(), artist.tolist(), genre.tolist())))
    return fu, fi


def rows(rng, n):
    u = rng.integers(0, a.users, n, dtype=np.uint32)
    i = rng.integers(0, a.items, n, dtype=np.uint32)
    r = rng.integers(1, 6, n).astype(np.float32)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)   # 4 distinct ids per row
    per = NG + 2
    row_ptr = np.empty(3 * n + 1, np.int64)
    base = per * np.arange(n, dtype=np.int64)
    row_ptr[0:3 * n:3] = base; row_ptr[1:3 * n:3] = base + NG; row_ptr[2:3 * n:3] = base + NG + 1; row_ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = u; idx[:, NG + 1] = i
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    return CSRData(r, row_ptr.astype(np.int32), idx.ravel(), val.ravel())


def trainer(extra, knobs, fu, fi):
    t = sa.Trainer(0, 0)
    t.seed(10)
    conf = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("wd_global", "0.001"),
            ("num_item", NI), ("num_user", NU), ("num_global", G), ("num_factor", a.factor), ("feature_user", fu), ("feature_item", fi)] + extra
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


WIN = [("amd:step", "minibatch"), ("amd:shared_user_from", a.users)]
SCHEMES = []
for s in a.schemes.split(","):
    if s == "exact":
        SCHEMES.append(("exact", [], []))
    elif s == "window":
        SCHEMES.append(("window, default rule", WIN, []))
    elif s:
        SCHEMES.append(("window, window_per_target_child %d" % int(s), WIN, [("window_per_target_child", int(s))]))

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


seeds = [int(s) for s in a.seeds.split(",")]
perf, drmse = {}, {}
with tempfile.TemporaryDirectory() as tmp:
    for si, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        fu, fi = tables(rng, tmp)
        d, test = rows(rng, a.n), rows(rng, a.test)
        rm = {}
        for name, extra, knobs in SCHEMES:
            t = trainer(extra, knobs, fu, fi)
            t0 = time.perf_counter()
            ds = t.dataset_from_csr(d)
            t.synchronize()
            build = time.perf_counter() - t0
            timed = []
            for p in range(a.passes):
                t0 = time.perf_counter()
                t.train_dataset(ds)
                t.synchronize()
                timed.append(time.perf_counter() - t0)
            pred = t.predict_batch(test)
            rm[name] = float(np.sqrt(np.mean((pred.astype(np.float64) - test.row_label) ** 2)))
            if si == 0:
                dt = float(np.mean(timed[1:])) if len(timed) > 1 else timed[0]
                perf[name] = dict(inst_per_s=a.n / dt, ms_per_pass=dt * 1e3, windows=ds.num_batches if ds.kind == 8 else 0, kind=ds.kind, build_s=build)
            print(json.dumps({"seed": seed, "scheme": name, "rmse": rm[name], "pass_ms": [x * 1e3 for x in timed], "kind": ds.kind,
                              "batches": ds.num_batches, "build_s": build}), file=sys.stderr, flush=True)
            ds.close(); t.close()
        if "exact" in rm and not a.no_drmse:
            for name, _, _ in SCHEMES:
                if name != "exact":
                    drmse.setdefault(name, []).append(rm[name] - rm["exact"])

out("# Side-feature variant (SURVEY 8(d2)) through feature_user / feature_item tables in the window step\n")
out("%d rows per pass, %d users (+ %d buckets + %d regions through feature_user), %d tracks (+ %d albums, %d artists, %d genres through "
    "feature_item), 4 of %d globals, k = %d; %d passes; held-out %d rows; seeds %s.  tools/sidetable_window.py\n"
    % (a.n, a.users, NB, NR, a.items, NAL, NAR, NGE, G, a.factor, a.passes, a.test, a.seeds))
out("| scheme | ms / pass | inst/s | windows / pass | vs exact | data set build s |")
out("|---|---|---|---|---|---|")
ex = perf["exact"]["inst_per_s"] if "exact" in perf else None
for name, _, _ in SCHEMES:
    p = perf[name]
    out("| %s | %.1f | %.3g M | %s | %s | %.1f |" % (name, p["ms_per_pass"], p["inst_per_s"] / 1e6, p["windows"] or "-",
                                                  "%.1fx" % (p["inst_per_s"] / ex) if ex else "-", p["build_s"]))
if drmse:
    out("\n| scheme | dRMSE seed " + " | dRMSE seed ".join(str(s) for s in seeds) + " | max abs |")
    out("|---|" + "---|" * (len(seeds) + 1))
    for name, v in drmse.items():
        out("| %s | %s | %.2e |" % (name, " | ".join("%+.2e" % x for x in v), max(abs(x) for x in v)))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")

#!/usr/bin/env python3
"""Calibration and speed of the ordered sub-steps for hot ITEM rows on the csr path of the one-GPU window step (knobs window_item_sub /
window_item_max), on one MI355X.  Two variants (k = 64, 3 passes), modelled on tools/shared_hot_window.py:

  A   Zipf(0.7) items (benchlib/orders.py: the stream of section 6h) with the four SURVEY 8(d2) globals of 10 K per row, so that the rows take
      wseq_from_csr: 4 globals, the user, the item.  No amd:shared_user_from.
  B   the section 6j variant: 64 buckets + 16 regions per user through feature_user, album / artist / genre per track through feature_item,
      uniform items; --shared-sub S runs it with window_shared_sub = S in every window-step setting.

Per variant: the exact pass, the parent's rule (window_item_sub = 0) --repeats times on the first seed so that the run-to-run spread of the
timing is on the page, and the grid --subs x --maxes.  Windows, ms and inst/s per pass (first seed, passes 2 .. 3), held-out dRMSE against the
exact pass for every data seed, whether the setting holds the contract (|dRMSE| <= 1e-4 on every seed), and its speed against the parent's rule.
--lib PATH loads another build of the library (the parent commit's, for the A/B of the parent's rule: run with --subs none there).
usage: python tools/item_hot_window.py --variant A --n 2000000 --subs 8,24,128 --maxes 128,256,512,1024,2048 --out FILE.md"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdfeature_amd as sa
from svdfeature_amd import CSRData

ap = argparse.ArgumentParser()
ap.add_argument("--variant", choices=["A", "B"], default="A")
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--test", type=int, default=200_000)
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--factor", type=int, default=64)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--seeds", default="1,2,3")
ap.add_argument("--subs", default="8,24,128", help="window_item_sub values; 'none': the exact pass and the parent's rule only")
ap.add_argument("--maxes", default="128,256,512,1024,2048")
ap.add_argument("--shared-sub", type=int, default=0, help="variant B: window_shared_sub of every window-step setting")
ap.add_argument("--repeats", type=int, default=3, help="timing runs of the parent's rule on the first seed")
ap.add_argument("--lib", default="", help="another build of libsvdfeature_amd.so (it need not know the knobs when --subs none)")
ap.add_argument("--label", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.lib:
    sa.LIB_PATH = os.path.abspath(a.lib)
B = a.variant == "B"
NG, G = 4, 10000
NB, NR = 64, 16
NAL, NAR, NGE = 10000, 2000, 256
NU = a.users + (NB + NR if B else 0)
NI = a.items + (NAL + NAR + NGE if B else 0)
subs = [] if a.subs == "none" else [int(x) for x in a.subs.split(",")]
maxes = [int(x) for x in a.maxes.split(",")]


def tables(rng, tmp):
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


def as_rows(rng, u, i, r):
    n = len(u)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)   # 4 distinct ids per row
    per = NG + 2
    row_ptr = np.empty(3 * n + 1, np.int64)
    base = per * np.arange(n, dtype=np.int64)
    row_ptr[0:3 * n:3] = base; row_ptr[1:3 * n:3] = base + NG; row_ptr[2:3 * n:3] = base + NG + 1; row_ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = u; idx[:, NG + 1] = i
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    return CSRData(r.astype(np.float32), row_ptr.astype(np.int32), idx.ravel(), val.ravel())


def data(seed):
    rng = np.random.default_rng(seed)
    n = a.n + a.test
    if B:
        u = rng.integers(0, a.users, n, dtype=np.uint32)
        i = rng.integers(0, a.items, n, dtype=np.uint32)
        r = rng.integers(1, 6, n).astype(np.float32)
    else:
        import bench
        from benchlib import orders
        u, i, r = orders.synth_zipf_triples(types.SimpleNamespace(Planted=bench.Planted), n, a.users, a.items, 4321 + seed)
    return rng, as_rows(rng, u[:a.n], i[:a.n], r[:a.n]), as_rows(rng, u[a.n:], i[a.n:], r[a.n:])


def trainer(extra, knobs, files):
    t = sa.Trainer(0, 0)
    t.seed(10)
    conf = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("wd_global", "0.001"),
            ("num_item", NI), ("num_user", NU), ("num_global", G), ("num_factor", a.factor)] + files + extra
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


WIN = [("amd:step", "minibatch")] + ([("amd:shared_user_from", a.users)] if B else [])
OTHER = [("window_shared_sub", a.shared_sub)] if B and a.shared_sub else []
ZERO = [("window_item_sub", 0)] if subs else []   # (a library without the knob: never named)
PARENT = "parent's rule (window_item_sub 0)"
SCHEMES = [("exact", [], [], True), (PARENT, WIN, OTHER + ZERO, True)]
SCHEMES += [("%s, timing run %d" % (PARENT, j + 2), WIN, OTHER + ZERO, False) for j in range(a.repeats - 1)]
SCHEMES += [("sub %d, max %d" % (s, m), WIN, OTHER + [("window_item_sub", s), ("window_item_max", m)], True) for s in subs for m in maxes]

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


seeds = [int(s) for s in a.seeds.split(",")]
perf, drmse = {}, {}
with tempfile.TemporaryDirectory() as tmp:
    for si, seed in enumerate(seeds):
        rng, d, test = data(seed)
        files = []
        if B:
            fu, fi = tables(rng, tmp)
            files = [("feature_user", fu), ("feature_item", fi)]
        rm, seen = {}, {}
        for name, extra, knobs, every_seed in SCHEMES:
            if si > 0 and not every_seed:
                continue
            t = trainer(extra, knobs, files)
            t0 = time.perf_counter()
            ds = t.dataset_from_csr(d)
            t.synchronize()
            build = time.perf_counter() - t0
            key = (ds.kind, ds.num_batches, dict(knobs).get("window_item_sub", 0))
            if si > 0 and name != "exact" and key in seen:   # the same windows and sub-step as a setting already run: the same bits
                rm[name] = rm[seen[key]]
                ds.close(); t.close()
                continue
            timed = []
            for p in range(a.passes):
                t0 = time.perf_counter()
                t.train_dataset(ds)
                t.synchronize()
                timed.append(time.perf_counter() - t0)
            pred = t.predict_batch(test)
            rm[name] = float(np.sqrt(np.mean((pred.astype(np.float64) - test.row_label) ** 2)))
            seen.setdefault(key, name)
            if si == 0:
                dt = float(np.mean(timed[1:])) if len(timed) > 1 else timed[0]
                perf[name] = dict(inst_per_s=a.n / dt, ms_per_pass=dt * 1e3, windows=ds.num_batches if ds.kind == 8 else 0, build_s=build)
            print(json.dumps({"seed": seed, "scheme": name, "rmse": rm[name], "pass_ms": [x * 1e3 for x in timed], "kind": ds.kind,
                              "batches": ds.num_batches, "build_s": build}), file=sys.stderr, flush=True)
            ds.close(); t.close()
        for name, _, _, every_seed in SCHEMES[1:]:
            if every_seed:
                drmse.setdefault(name, []).append(rm[name] - rm["exact"])

par = [perf[n]["ms_per_pass"] for n in perf if n.startswith(PARENT)]
par_ms, spread = float(np.mean(par)), (max(par) - min(par)) / float(np.mean(par))
out("## Variant %s, %d rows per pass%s\n" % ("B (feature_user / feature_item tables, section 6j)" if B else "A (Zipf(0.7) items + 4 of 10 K globals)", a.n,
                                            (" -- " + a.label) if a.label else ""))
out("%d users%s, %d items%s, 4 of %d globals, k = %d; %d passes; held-out %d rows; seeds %s%s.  tools/item_hot_window.py\n"
    % (a.users, " + %d buckets + %d regions (feature_user)" % (NB, NR) if B else "", a.items,
       " (+ %d albums, %d artists, %d genres through feature_item)" % (NAL, NAR, NGE) if B else " ~ Zipf(0.7)", G, a.factor, a.passes, a.test, a.seeds,
       "; window_shared_sub = %d" % a.shared_sub if OTHER else ""))
out("Parent's rule, %d timing runs on seed %d: %s ms per pass (mean %.1f, spread %.1f %%).\n"
    % (len(par), seeds[0], " / ".join("%.1f" % x for x in par), par_ms, 100 * spread))
out("| setting | windows / pass | ms / pass | inst/s | vs parent's rule | dRMSE seed " + " | dRMSE seed ".join(str(s) for s in seeds) + " | max abs | holds 1e-4 |")
out("|---|---|---|---|---|" + "---|" * (len(seeds) + 2))
best = None
for name, _, _, every_seed in SCHEMES:
    p = perf[name]
    if name == "exact":
        out("| exact | - | %.1f | %.3g M | %.2fx |%s - | - |" % (p["ms_per_pass"], p["inst_per_s"] / 1e6, par_ms / p["ms_per_pass"], " - |" * len(seeds)))
        continue
    if not every_seed:
        continue
    v = drmse[name]
    worst = max(abs(x) for x in v)
    holds = worst <= 1e-4
    out("| %s | %d | %.1f | %.3g M | %.2fx | %s | %.2e | %s |" % (name, p["windows"], p["ms_per_pass"], p["inst_per_s"] / 1e6, par_ms / p["ms_per_pass"],
                                                               " | ".join("%+.2e" % x for x in v), worst, "yes" if holds else "NO"))
    if holds and name != PARENT and (best is None or p["ms_per_pass"] < perf[best]["ms_per_pass"]):
        best = name
if subs:
    if best is None:
        out("\nNo setting of the grid holds |dRMSE| <= 1e-4 on every seed.")
    else:
        gain = par_ms / perf[best]["ms_per_pass"]
        out("\nFastest setting that holds |dRMSE| <= 1e-4 on every seed: %s, %.2fx the parent's rule (run-to-run spread of the parent's timing: %.1f %%)%s."
            % (best, gain, 100 * spread, "" if gain > 1 + spread else " -- NOT beyond that spread"))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")

#!/usr/bin/env python3
"""Calibration and speed of the ordered sub-steps for hot items of rank pairs in the one-GPU window step (knobs window_pair_sub /
window_pair_max), on one MI355X, modelled on tools/item_hot_window.py.

Data: the BASELINE configs[4] model shape as bench.py sets it for `pairwise` (sigmoid rank loss, no user bias, k = 128); users uniform, both
items of a pair ~ Zipf(0.7) over a permuted catalogue and distinct (--uniform: uniform items), the positive item the one the planted model
(+ noise) scores higher (benchlib/orders.py: synth_generator_pairs' choice), random order.

Default mode: the exact pass, the parent's rule (window_pair_sub = 0) and the grid --subs x --maxes.  Per setting: windows per pass, the median
ms per pass over --time-passes passes (first seed), and for every data seed the held-out pair accuracy and mean margin after --passes passes
against the exact run of the same passes over the same rows.  The project's pair contract (benchlib/orders.py) is accuracy within 3e-3 and
margin within 2 %; `of contract` is the larger of the two ratios, worst seed.

--subs none: the exact pass is skipped and only the window step with the knobs never named is run -- the run a library without the knobs
understands: --lib PATH loads another build (the parent commit's) for the A/B of the default path; the line ends with a checksum of the model
so that equal bits can be seen across the two.
usage: python tools/pair_hot_window.py --n 20000000 --subs 8,24,128 --maxes 512,1024,2048,4096 --out FILE.md"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import svdfeature_amd as sa
from benchlib.synth import Planted

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=20_000_000)
ap.add_argument("--test", type=int, default=200_000)
ap.add_argument("--users", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=100_000)
ap.add_argument("--factor", type=int, default=128)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--time-passes", type=int, default=7)
ap.add_argument("--seeds", default="1,2,3")
ap.add_argument("--subs", default="8,24,128", help="window_pair_sub values; 'none': the window step with the knobs never named")
ap.add_argument("--maxes", default="512,1024,2048,4096")
ap.add_argument("--uniform", action="store_true", help="uniform items instead of Zipf(0.7)")
ap.add_argument("--no-exact", action="store_true", help="skip the exact pass (speed only)")
ap.add_argument("--lib", default="", help="another build of libsvdfeature_amd.so (it need not know the knobs when --subs none)")
ap.add_argument("--label", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.lib:
    sa.LIB_PATH = os.path.abspath(a.lib)
subs = [] if a.subs == "none" else [int(x) for x in a.subs.split(",")]
maxes = [int(x) for x in a.maxes.split(",")]
ZIPF = 0.7


def data(seed):
    rng = np.random.default_rng(9000 + seed)
    n = a.n + a.test
    u = rng.integers(0, a.users, n, dtype=np.uint32)
    if a.uniform:
        x = rng.integers(0, a.items, n, dtype=np.uint32)
        y = ((x.astype(np.int64) + 1 + rng.integers(0, a.items - 1, n)) % a.items).astype(np.uint32)
    else:
        w = 1.0 / np.arange(1, a.items + 1, dtype=np.float64) ** ZIPF
        cdf = np.cumsum(w / w.sum())
        perm = rng.permutation(a.items).astype(np.uint32)
        draw = lambda m: np.minimum(np.searchsorted(cdf, rng.random(m)), a.items - 1)   # noqa: E731
        rx, ry = draw(n), draw(n)
        same = np.nonzero(rx == ry)[0]
        while len(same):   # distinct items: the second one drawn again
            ry[same] = draw(len(same))
            same = same[rx[same] == ry[same]]
        x, y = perm[rx], perm[ry]
    pl = Planted(a.users, a.items, rng)
    first = pl.score(u, x) + 0.35 * rng.standard_normal(n).astype(np.float32) > pl.score(u, y)
    pos, neg = np.where(first, x, y).astype(np.uint32), np.where(first, y, x).astype(np.uint32)
    return (u[:a.n], pos[:a.n], neg[:a.n]), sa.pairs_as_csr(u[a.n:], pos[a.n:], neg[a.n:])


def trainer(extra, knobs):
    t = sa.Trainer(0, 3)
    t.seed(10)
    conf = [("base_score", "0.5"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("num_item", a.items), ("num_user", a.users),
            ("num_global", "0"), ("num_factor", a.factor), ("active_type", "3"), ("no_user_bias", "1")] + extra
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    for k, v in knobs:
        t.set_knob(k, v)
    return t


WIN = [("amd:step", "minibatch")]
PARENT = "parent's rule" + (" (window_pair_sub 0)" if subs else " (knobs never named)")
SCHEMES = ([] if (a.no_exact or not subs) else [("exact", [], [])]) + [(PARENT, WIN, [("window_pair_sub", 0)] if subs else [])]
SCHEMES += [("sub %d, max %d" % (s, m), WIN, [("window_pair_sub", s), ("window_pair_max", m)]) for s in subs for m in maxes]
have_exact = SCHEMES[0][0] == "exact"

lines = []


def out(s):
    print(s, flush=True)
    lines.append(s)


seeds = [int(s) for s in a.seeds.split(",")]
perf, acc, margin, sums = {}, {}, {}, {}
for si, seed in enumerate(seeds):
    cols, test = data(seed)
    for name, extra, knobs in SCHEMES:
        t = trainer(extra, knobs)
        t0 = time.perf_counter()
        ds = t.dataset_from_pairs(*cols)
        t.synchronize()
        build = time.perf_counter() - t0
        timed = []
        for p in range(a.passes):
            t0 = time.perf_counter()
            t.train_dataset(ds)
            t.synchronize()
            timed.append(time.perf_counter() - t0)
        pred = t.predict_batch(test)
        acc.setdefault(name, []).append(float(np.mean(pred > 0)))
        margin.setdefault(name, []).append(float(np.mean(pred, dtype=np.float64)))
        if not have_exact:
            sums.setdefault(name, []).append("%08x" % zlib.crc32(t.view("W_item").tobytes() + t.view("W_user").tobytes() + t.view("i_bias").tobytes()))
        if si == 0:
            for p in range(a.passes, a.time_passes + 1):   # (the first pass of all warms up and is left out)
                t0 = time.perf_counter()
                t.train_dataset(ds)
                t.synchronize()
                timed.append(time.perf_counter() - t0)
            ms = np.array(timed[1:]) * 1e3
            perf[name] = dict(ms=float(np.median(ms)), lo=float(ms.min()), hi=float(ms.max()), windows=ds.num_batches if ds.kind == 8 else 0, build_s=build)
        print(json.dumps({"seed": seed, "scheme": name, "accuracy": acc[name][-1], "margin": margin[name][-1], "pass_ms": [x * 1e3 for x in timed],
                          "kind": ds.kind, "batches": ds.num_batches, "build_s": build}), file=sys.stderr, flush=True)
        ds.close(); t.close()

par_ms = perf[PARENT]["ms"]
out("## %s items, %d pairs per pass%s\n" % ("Uniform" if a.uniform else "Zipf(0.7)", a.n, (" -- " + a.label) if a.label else ""))
out("%d users, %d items, k = %d, sigmoid rank loss, no user bias; accuracy after %d passes on %d held-out pairs, seeds %s; ms per pass = median of passes 2 .. %d on "
    "seed %d (min .. max beside it).  tools/pair_hot_window.py\n" % (a.users, a.items, a.factor, a.passes, a.test, a.seeds, len(ms) + 1, seeds[0]))
if have_exact:
    out("| setting | windows / pass | ms / pass | G pairs/s | vs parent's rule | d accuracy, seeds " + ", ".join(str(s) for s in seeds) + " | d margin (relative) | of contract |")
    out("|---|---|---|---|---|---|---|---|")
else:
    out("| setting | windows / pass | ms / pass | G pairs/s | accuracy | margin | model crc32, seeds " + ", ".join(str(s) for s in seeds) + " |")
    out("|---|---|---|---|---|---|---|")
for name, _, _ in SCHEMES:
    p = perf[name]
    head = "| %s | %s | %.1f (%.1f .. %.1f) | %.3f |" % (name, p["windows"] or "-", p["ms"], p["lo"], p["hi"], a.n / p["ms"] / 1e6)
    if not have_exact:
        out(head + " %s | %s | %s |" % (" / ".join("%.5f" % x for x in acc[name]), " / ".join("%.5f" % x for x in margin[name]), " / ".join(sums[name])))
    elif name == "exact":
        out(head + " %.2fx | (%s) | (%s) | - |" % (par_ms / p["ms"], " / ".join("%.5f" % x for x in acc[name]), " / ".join("%.5f" % x for x in margin[name])))
    else:
        da = [x - e for x, e in zip(acc[name], acc["exact"])]
        dm = [(x - e) / abs(e) for x, e in zip(margin[name], margin["exact"])]
        of = max(max(abs(x) for x in da) / 3e-3, max(abs(x) for x in dm) / 0.02)
        out(head + " %.2fx | %s | %s | %.0f %% |" % (par_ms / p["ms"], " / ".join("%+.1e" % x for x in da), " / ".join("%+.2f %%" % (100 * x) for x in dm), 100 * of))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")

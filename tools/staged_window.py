#!/usr/bin/env python3
"""`amd:step` on the staged route, measured through the reference's own CLI linked against the engine (oracle/_ref/svd_feature_amd; DESIGN.md
section 6l): the binary drives ISVDTrainer::update() one virtual call at a time, the handle trains every chunk of staged rows.

  throughput   inst/s of the CLI under: default (exact), amd:step = minibatch, amd:step = auto, on four inputs; every cell is timed over a
               window of about --target seconds (the rounds are sized per cell) and repeated --reps times with the settings alternating
                 pairs     a user-group buffer through input_type = 2 (PairwiseRankGenerator: the generator's order)
                 sidefeat  the SURVEY 8(d2) side-feature variant (4 globals, user, bucket id as a shared user entry, item), CSR buffer
                 blocks    user-group blocks with implicit feedback (demo/implicitFeedback shape)
                 plain     uniform plain ratings, CSR buffer
               window = wall time of R rounds minus the wall time of a run with num_round = 0 (start-up, model init, first save); the share of the
               handle's flush time (schedule / build + upload + launch: SVDF_PROFILE) in it, and its parts
  ab           the DEFAULT route against another build of the library (--parent-cli: the same CLI next to the parent commit's library),
               alternating runs sized the same way, median of 7
  accuracy     ML-100K through the CLI at 5 and 40 rounds: test RMSE of amd:step = minibatch against the exact run
  trace        (not in the default set) one rocprofv3 --kernel-trace --stats run per input under amd:step = minibatch: GPU kernel time against wall time

usage: python tools/staged_window.py [--only throughput,ab,accuracy,trace] [--parent-cli PATH] [--out profiles/r10_staged_window.md]"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svdfeature_amd as sa
from svdfeature_amd import CSRData
from svdfeature_amd import data as D

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="throughput,ab,accuracy")
ap.add_argument("--cli", default=os.path.join(ROOT, "oracle", "_ref", "svd_feature_amd"))
ap.add_argument("--parent-cli", default="")
ap.add_argument("--rounds", type=int, default=3, help="rounds of the trace runs")
ap.add_argument("--target", type=float, default=2.0, help="throughput / ab: seconds the timed window of a cell should last")
ap.add_argument("--reps", type=int, default=5, help="throughput / ab: repetitions per cell")
ap.add_argument("--n", type=int, default=2_000_000, help="rows of the sidefeat / plain inputs")
ap.add_argument("--pair-users", type=int, default=6000)
ap.add_argument("--block-users", type=int, default=20000)
ap.add_argument("--factor", type=int, default=64)
ap.add_argument("--out", default="")
a = ap.parse_args()
only = set(a.only.split(","))
a.cli = os.path.abspath(a.cli)
a.parent_cli = os.path.abspath(a.parent_cli) if a.parent_cli else ""
lines = []


def out(s=""):
    print(s, flush=True)
    lines.append(s)


def write_conf(path, pairs):
    with open(path, "w") as f:
        for k, v in pairs:
            f.write('%s = %s\n' % (k, ('"%s"' % v) if k in ("buffer_feature", "model_out_folder") else v))


def run_cli(cli, workdir, rounds, extra=(), timeout=900):
    """one CLI run; returns wall seconds and what SVDF_PROFILE printed (flush seconds, instances, staged chunks)"""
    env = dict(os.environ, SVDF_PROFILE="1", SVDF_QUIET="1")
    t0 = time.perf_counter()
    p = subprocess.run([cli, "run.conf", "num_round=%d" % rounds, "silent=1"] + list(extra), cwd=workdir, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    wall = time.perf_counter() - t0
    text = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (cli, p.returncode, text[-2000:]))
    m = re.search(r"flush \(schedule\+upload\+launch\) ([0-9.]+)s\s+model save/load ([0-9.]+)s\s+instances (\d+) flushes (\d+)", text)
    s = re.search(r"staged route: (\d+) chunks trained by the window step, (\d+) kept exact.*window build ([0-9.]+)s.*host regrouping ([0-9.]+)s, allocations \+ uploads \+ "
                  r"synchronisations ([0-9.]+)s.*pool (\d+), from hipMalloc (\d+)", text)
    return dict(wall=wall, flush=float(m.group(1)) if m else 0.0, model=float(m.group(2)) if m else 0.0, instances=int(m.group(3)) if m else 0,
                flushes=int(m.group(4)) if m else 0, window_chunks=int(s.group(1)) if s else 0, exact_chunks=int(s.group(2)) if s else 0,
                build=float(s.group(3)) if s else 0.0, host=float(s.group(4)) if s else 0.0, adopt=float(s.group(5)) if s else 0.0,
                pool_taken=int(s.group(6)) if s else 0, pool_missed=int(s.group(7)) if s else 0)


BASE = [("base_score", "3"), ("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("active_type", "0")]


def input_pairs(d):
    """binary feedback per user, no implicit-feedback list (demo/pairwiseRank): the generator draws the pairs of a user block in a row"""
    nu, ni, rng = a.pair_users, 1682, np.random.default_rng(1)
    blocks = []
    e = np.zeros(0, np.uint32), np.zeros(0, np.float32)
    for u in range(nu):
        it = rng.choice(ni, size=40, replace=False).astype(np.uint32)
        lab = (rng.random(40) < 0.5).astype(np.float32)
        blocks.append(D.PlusBlock(e[0], e[1], CSRData.from_triples(np.full(40, u, np.uint32), it, lab), D.TAG_DEFAULT))
    D.write_ugroup_buffer(os.path.join(d, "train.buffer"), blocks)
    return [("learning_rate", "0.005"), ("wd_item", "0.004"), ("wd_user", "0.004"), ("active_type", "3"), ("no_user_bias", "1"), ("input_type", "2"),
            ("format_type", "1"), ("num_user", nu), ("num_item", ni), ("num_ufeedback", ni), ("num_global", 0), ("num_factor", a.factor)], []


def input_sidefeat(d):
    n, users, items, NG, G, NB, rng = a.n, 1_000_000, 100_000, 4, 10000, 64, np.random.default_rng(2)
    u = rng.integers(0, users, n, dtype=np.uint32)
    g = (rng.integers(0, G // NG, (n, NG)) + np.arange(NG) * (G // NG)).astype(np.uint32)
    per = NG + 3
    base = per * np.arange(n, dtype=np.int64)
    ptr = np.empty(3 * n + 1, np.int64)
    ptr[0:3 * n:3] = base; ptr[1:3 * n:3] = base + NG; ptr[2:3 * n:3] = base + NG + 2; ptr[3 * n] = per * n
    idx = np.empty((n, per), np.uint32); idx[:, :NG] = g; idx[:, NG] = u; idx[:, NG + 1] = users + (u % NB); idx[:, NG + 2] = rng.integers(0, items, n)
    val = np.ones((n, per), np.float32); val[:, :NG] = rng.uniform(0, 1, (n, NG))
    D.write_csr_buffer(os.path.join(d, "train.buffer"), CSRData(rng.integers(1, 6, n).astype(np.float32), ptr.astype(np.int32), idx.ravel(), val.ravel()),
                       batch_size=10000)
    return BASE + [("wd_global", "0.001"), ("num_user", users + NB), ("num_item", items), ("num_global", G), ("num_factor", a.factor)], ["amd:shared_user_from=%d" % users]


def input_blocks(d):
    nu, ni, rng = a.block_users, 20000, np.random.default_rng(3)
    blocks = []
    for u in range(nu):
        it = rng.integers(0, ni, 50).astype(np.uint32)
        fb = np.unique(it)
        blocks.append(D.PlusBlock(fb, np.full(len(fb), 1.0 / np.sqrt(len(fb)), np.float32),
                                  CSRData.from_triples(np.full(50, u, np.uint32), it, rng.integers(1, 6, 50).astype(np.float32)), D.TAG_DEFAULT))
    D.write_ugroup_buffer(os.path.join(d, "train.buffer"), blocks)
    return BASE + [("format_type", "1"), ("num_user", nu), ("num_item", ni), ("num_ufeedback", ni), ("wd_ufeedback", "0.004"), ("num_global", 0),
                   ("num_factor", a.factor)], []


def input_plain(d):
    n, nu, ni, rng = a.n, 200_000, 60_000, np.random.default_rng(4)
    D.write_csr_buffer(os.path.join(d, "train.buffer"), CSRData.from_triples(rng.integers(0, nu, n), rng.integers(0, ni, n), rng.integers(1, 6, n).astype(np.float32)),
                       batch_size=10000)
    return BASE + [("num_user", nu), ("num_item", ni), ("num_global", 0), ("num_factor", a.factor)], []


SETTINGS = [("default (exact)", []), ("amd:step = minibatch", ["amd:step=minibatch"]), ("amd:step = auto", ["amd:step=auto"])]

def timed_cells(d, always, settings, clis=None):
    """every setting of one input: rounds sized so that the timed window (wall of R rounds minus wall of a num_round = 0 run of the same setting) is
    about --target seconds, --reps repetitions with the settings alternating; per setting the list of per-repetition results"""
    clis = clis or {name: a.cli for name, _ in settings}
    rounds = {}
    for name, extra in settings:   # one short run to size the rounds
        z = run_cli(clis[name], d, 0, extra + always)
        r = run_cli(clis[name], d, 3, extra + always)
        per_round = max((r["wall"] - z["wall"]) / 3, 1e-4)
        rounds[name] = int(min(max(3, np.ceil(a.target / per_round)), 400))
    res = {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, extra in settings:
            z = run_cli(clis[name], d, 0, extra + always)
            r = run_cli(clis[name], d, rounds[name], extra + always)
            w = max(r["wall"] - z["wall"], 1e-9)
            res[name].append(dict(window=w, rate=r["instances"] / w, rps=rounds[name] / w, inst=r["instances"] / rounds[name], flush=r["flush"] / w,
                                  build=r["build"] / w, host=r["host"] / w, adopt=r["adopt"] / w, wc=r["window_chunks"], ec=r["exact_chunks"],
                                  pool=r["pool_taken"], malloc=r["pool_missed"], rounds=rounds[name]))
    return res


def med(v, k):
    return statistics.median(x[k] for x in v)


if "throughput" in only:
    out("## Throughput of oracle/_ref/svd_feature_amd (the reference's CLI, one update() call per instance / block)\n")
    out("Per cell: rounds sized so that the timed window -- wall time of the run minus the wall time of a num_round = 0 run of the same setting (start-up, "
        "model init, first save) -- is about %.0f s; %d repetitions, the three settings alternating; median and [min .. max] of the repetitions.  "
        "flush = the handle's flush time (per-chunk schedule or window build + upload + launch, host timers) over the window; build = the per-chunk "
        "pre-check + window build inside it; for user-unit windows split into host regrouping and the windows' allocations + uploads + synchronisations.  "
        "`clear` = the setting's slowest repetition is faster than the default's fastest (or its fastest slower than the default's slowest).  k = %d\n"
        % (a.target, a.reps, a.factor))
    out("| input | setting | rounds | window s | inst / round | M inst/s median [min .. max] | vs default | clear | flush | build | host regroup | alloc+upload+sync | blocks pool / hipMalloc | window / exact chunks |")
    out("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for name, make in (("pairs (input_type = 2)", input_pairs), ("sidefeat (SURVEY d2, 2 M rows)", input_sidefeat), ("blocks (SVD++)", input_blocks),
                       ("plain ratings (uniform)", input_plain)):
        with tempfile.TemporaryDirectory() as d:
            conf, always = make(d)
            write_conf(os.path.join(d, "run.conf"), conf + [("buffer_feature", "train.buffer"), ("model_out_folder", "./")])
            res = timed_cells(d, always, SETTINGS)
            base = res[SETTINGS[0][0]]
            blo, bhi = min(x["rate"] for x in base), max(x["rate"] for x in base)
            for sname, _ in SETTINGS:
                v = res[sname]
                lo, hi = min(x["rate"] for x in v), max(x["rate"] for x in v)
                clear = "-" if v is base else ("yes" if lo > bhi or hi < blo else "no")
                out("| %s | %s | %d | %.2f | %d | %.2f [%.2f .. %.2f] | %.2fx | %s | %.0f %% | %.0f %% | %.0f %% | %.0f %% | %d / %d | %d / %d |" %
                    (name, sname, v[0]["rounds"], med(v, "window"), med(v, "inst"), med(v, "rate") / 1e6, lo / 1e6, hi / 1e6, med(v, "rate") / med(base, "rate"), clear,
                     100 * med(v, "flush"), 100 * med(v, "build"), 100 * med(v, "host"), 100 * med(v, "adopt"), v[0]["pool"], v[0]["malloc"], v[0]["wc"], v[0]["ec"]))
    out()

if "trace" in only:
    import csv
    import glob
    out("## GPU work under amd:step = minibatch (rocprofv3 --kernel-trace --stats, a run of its own per input, %d rounds)\n" % a.rounds)
    out("| input | kernel time per round ms | dispatches per round | busiest kernels (share of kernel time) |")
    out("|---|---|---|---|")
    for name, make in (("pairs (input_type = 2)", input_pairs), ("sidefeat (SURVEY d2)", input_sidefeat), ("blocks (SVD++)", input_blocks),
                       ("plain ratings (uniform)", input_plain)):
        with tempfile.TemporaryDirectory() as d:
            conf, always = make(d)
            write_conf(os.path.join(d, "run.conf"), conf + [("buffer_feature", "train.buffer"), ("model_out_folder", "./")])
            t0 = time.perf_counter()
            p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(d, "kt"), "-o", "kt", "--",
                                a.cli, "run.conf", "num_round=%d" % a.rounds, "silent=1", "amd:step=minibatch"] + always, cwd=d,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stdout.decode(errors="replace")[-2000:])
            per = {}
            for f in glob.glob(os.path.join(d, "kt", "**", "*kernel_trace.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
                    c = per.setdefault(k, [0, 0])
                    c[0] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"]); c[1] += 1
            total = sum(v[0] for v in per.values()) * 1e-9
            top = sorted(per.items(), key=lambda kv: -kv[1][0])[:4]
            out("| %s | %.2f | %d | %s |" % (name, 1e3 * total / a.rounds, sum(v[1] for v in per.values()) // a.rounds,
                                             ", ".join("%s %.0f %%" % (k.replace("svdf::", "") or "(anonymous namespace)", 100.0 * v[0] * 1e-9 / max(total, 1e-12)) for k, v in top)))
    out()

if "pool" in only:
    out("## The handle's block pool (knob staged_pool) on the sidefeat rows, through the Python binding\n")
    with tempfile.TemporaryDirectory() as d:
        conf, always = input_sidefeat(d)
        data = D.read_csr_buffer(os.path.join(d, "train.buffer"))
    walls = {0: [], 1: []}
    for rep in range(3):
        for mode in (0, 1):
            t = sa.Trainer(0, 0)
            t.seed(10)
            for k, v in conf + [("amd:step", "minibatch"), ("amd:shared_user_from", 1_000_000)]:
                t.set_param(k, str(v))
            t.init_model(); t.init_trainer(); t.set_knob("staged_pool", mode)
            t.update_batch(data); t.finish_round(); t.synchronize()      # the first chunk fills the pool
            t0 = time.perf_counter()
            for _ in range(3):
                t.update_batch(data); t.finish_round()
            t.synchronize()
            walls[mode].append((time.perf_counter() - t0) / 3)
            t.close()
    for mode in (0, 1):
        out("staged_pool = %d: seconds per 2 M-row chunk, 3 repetitions alternating: %s; median %.3f" %
            (mode, " ".join("%.3f" % x for x in walls[mode]), statistics.median(walls[mode])))
    out()

if "ab" in only and a.parent_cli:
    out("## Default route: this library against the parent commit's, alternating runs\n")
    with tempfile.TemporaryDirectory() as d:
        conf, _ = input_plain(d)
        write_conf(os.path.join(d, "run.conf"), conf + [("buffer_feature", "train.buffer"), ("model_out_folder", "./")])
        a.reps, keep = 7, a.reps
        res = timed_cells(d, [], [("this", []), ("parent", [])], {"this": a.cli, "parent": a.parent_cli})
        a.reps = keep
        for who in ("this", "parent"):
            v = res[who]
            out("%s: %d rounds per run, timed window median %.2f s; M inst/s of the 7 runs: %s; median %.2f" %
                (who, v[0]["rounds"], med(v, "window"), " ".join("%.2f" % (x["rate"] / 1e6) for x in v), med(v, "rate") / 1e6))
        mt, mp_ = med(res["this"], "rate"), med(res["parent"], "rate")
        spread = lambda v: 100.0 * (max(x["rate"] for x in v) - min(x["rate"] for x in v)) / med(v, "rate")
        out("difference of the medians %+.2f %% (this against parent); run-to-run spread (max - min over median) this %.2f %%, parent %.2f %%\n" %
            (100.0 * (mt - mp_) / mp_, spread(res["this"]), spread(res["parent"])))

if "accuracy" in only:
    import cases
    out("## Accuracy: ML-100K (ua.base, k = 64) through the CLI, test RMSE on ua.test\n")
    base, test = cases.ml100k()
    out("| rounds | exact | amd:step = minibatch | dRMSE | window chunks |")
    out("|---|---|---|---|---|")
    for rounds in (5, 40):
        rm, chunks = {}, 0
        for sname, extra in SETTINGS[:2]:
            with tempfile.TemporaryDirectory() as d:
                D.write_csr_buffer(os.path.join(d, "train.buffer"), base)
                write_conf(os.path.join(d, "run.conf"), cases.BASICMF_CONF + [("buffer_feature", "train.buffer"), ("model_out_folder", "./")])
                r = run_cli(a.cli, d, rounds, extra)
                chunks = r["window_chunks"]
                t = sa.Trainer(0, 0)
                t.load_model(os.path.join(d, "%04d.model" % rounds))
                t.init_trainer()
                rm[sname] = cases.rmse(t.predict_batch(test), test.row_label)
                t.close()
        out("| %d | %.6f | %.6f | %+.2e | %d |" % (rounds, rm[SETTINGS[0][0]], rm[SETTINGS[1][0]], rm[SETTINGS[1][0]] - rm[SETTINGS[0][0]], chunks))
    out()

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")

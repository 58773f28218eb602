#!/usr/bin/env python3
"""Batch ranking evaluation on the live model (svdf_rank_eval_positions) against the route the parent had: save the
model, load it into a svdf_ranker, feed every user as tag lines (sa.Ranker.process_rows).  Results in profiles/r24_rank_eval.md.

Input: --sections users (10 000) against --items items (100 000) at one num_factor per invocation; each section has 3 positives and 100
banned items.  The model is trained by one pass of rank pairs first.  The save and the load (+ preparing the candidate matrix) are timed
separately and once; then the two routes alternate --reps times (5) on the same sections, and medians with the spread are reported.  The
positions of both routes are compared in the same run wherever the batch call reports no tie.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_eval.py --k 64 --out r24_k64.json && timeout -k 10 300 python tools/rank_eval.py --k 128 --out r24_k128.json

--only-batch runs the batch call alone (--reps times after one warm-up): the program to put behind `rocprofv3 --kernel-trace --stats --`
in a run of its own (the kernel time of k_rank_eval_sweep is then in the trace), and behind a counter collection in another."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_UNFUSED = 157.3e12 / 2.0   # the fp32 vector spec counts an FMA as two operations; an unfused mul + add pair issues at half of it
HBM_BYTES_PER_S = 8.0e12


def sections(S, nu, ni, seed):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    offs = rng.choice(ni, 103, replace=False)   # 103 distinct items per section: one random set of offsets rotated by a per-section base
    pick = ((rng.integers(0, ni, S)[:, None] + offs[None, :]) % ni).astype(np.uint32)
    pos_ptr = (3 * np.arange(S + 1)).astype(np.int64)
    ban_ptr = (100 * np.arange(S + 1)).astype(np.int64)
    return users, pos_ptr, np.ascontiguousarray(pick[:, :3]).ravel(), ban_ptr, np.ascontiguousarray(pick[:, 3:]).ravel()


def tag_lines(users, pick_pos, pick_ban):
    """USER, POS_SAMPLE, BAN_SAMPLE, PROCESS per section as one CSRData (ids travel in the user field)"""
    import svdfeature_amd as sa
    S = len(users)
    idx = np.concatenate([users[:, None], pick_pos.reshape(S, 3), pick_ban.reshape(S, 100)], axis=1).astype(np.uint32)
    base = 104 * np.arange(S, dtype=np.int64)[:, None]
    rp = np.concatenate([base + o for o in ([0, 0, 1], [1, 1, 4], [4, 4, 104], [104, 104, 104])], axis=1)   # (g, u, i) starts of the 4 rows
    row_ptr = np.concatenate([rp.ravel(), [104 * S]]).astype(np.int32)
    label = np.tile(np.array([2.0, 1.0, -1.0, 4.0], np.float32), S)
    return sa.CSRData(label, row_ptr, idx.ravel(), np.ones(idx.size, np.float32))


def item_lines(ni):
    import svdfeature_amd as sa
    rp = np.zeros(3 * ni + 1, np.int32)
    c = np.arange(ni)
    rp[0::3][:ni], rp[1::3], rp[2::3], rp[3::3] = c, c, c, c + 1
    return sa.CSRData(np.zeros(ni, np.float32), rp, c.astype(np.uint32), np.ones(ni, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--sections", type=int, default=10000)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    nu, ni, S, k = a.users, a.items, a.sections, a.k
    t = sa.Trainer(0, 3)
    t.seed(7)
    for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(1000000, nu, ni, seed=3)))
    t.synchronize()
    users, pos_ptr, pos_item, ban_ptr, ban_item = sections(S, nu, ni, seed=11)
    lists = (users, pos_ptr, pos_item, ban_ptr, ban_item)
    rec = {"k": k, "sections": S, "items": ni, "positives": 3, "banned": 100, "reps": a.reps}
    got = t.rank_positions(*lists)   # warm-up: buffers, code objects
    batch_s, ranker_s = [], []
    if a.only_batch:
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = t.rank_positions(*lists)
            batch_s.append(time.perf_counter() - t0)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "m.model")
            t0 = time.perf_counter()
            t.save_model(path)
            rec["save_s"] = time.perf_counter() - t0
            rec["model_bytes"] = os.path.getsize(path)
            t0 = time.perf_counter()
            r = sa.Ranker(0, 3)
            r.set_param("top_k", "0")
            r.load_model(path)
            r.init_ranker(ni)
            r.process_rows(item_lines(ni))
            rec["load_and_prepare_s"] = time.perf_counter() - t0
        lines = tag_lines(users, pos_item, ban_item)
        want = r.process_rows(lines)   # warm-up of the same kind
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = t.rank_positions(*lists)
            batch_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = r.process_rows(lines)
            ranker_s.append(time.perf_counter() - t0)
        position, tied = got[0], got[1]
        untied = tied == 0
        rec["positions_compared"] = int(untied.sum())
        rec["positions_equal"] = bool(np.array_equal(position[untied], want[untied]))
        rec["positions_tied"] = int((~untied).sum())
        rec["ranker_s"] = {"median": float(np.median(ranker_s)), "min": float(min(ranker_s)), "max": float(max(ranker_s))}
        rec["ranker_tiles"] = r.counter(3)
        rec["ranker_host_sorts"] = r.counter(1)
    med = float(np.median(batch_s))
    rec["batch_s"] = {"median": med, "min": float(min(batch_s)), "max": float(max(batch_s))}
    if ranker_s:
        rec["speedup_median"] = rec["ranker_s"]["median"] / med
    pitch = (k + 3) // 4 * 4
    ops = 2.0 * k * S * ni
    rec["call_ops_per_s"] = ops / med
    rec["call_share_of_unfused_fp32_peak"] = ops / med / PEAK_UNFUSED
    tiles = (S + 63) // 64
    rec["w_item_bytes_swept"] = float(tiles) * ni * pitch * 4
    rec["call_w_item_bytes_per_s"] = rec["w_item_bytes_swept"] / med
    rec["call_share_of_hbm_roofline"] = rec["call_w_item_bytes_per_s"] / HBM_BYTES_PER_S
    rec["nan_sections"] = int(got[3].sum())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not a.only_batch and not rec["positions_equal"]:
        sys.exit("rank_eval: the batch call and the ranker disagree on an untied position")


if __name__ == "__main__":
    main()

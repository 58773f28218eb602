#!/usr/bin/env python3
"""Top-N item lists on the live model (svdf_rank_topn) against the route the parent had to the same lists: save the
model, load it into a svdf_ranker with top_k set, feed every user as tag lines (sa.Ranker.process_rows).  Results in profiles/r25_rank_topn.md.

Input: tools/rank_eval.py's -- --sections users (10 000) against --items items (100 000) at one num_factor per invocation, 100 banned items
per section, the model trained by one pass of rank pairs first.  For every top_n of --top (10,100): the ranker's save and load (+ the
candidate matrix) are timed once; then the two routes alternate --reps times (5) on the same sections after a warm-up of each, and medians
with the spread are reported.  The lists of both routes are compared in the same run on every section whose top_n + 1 best scores are
strictly decreasing (found by asking the batch call for top_n + 1).

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_topn.py --k 64 --out r25_k64.json && timeout -k 10 300 python tools/rank_topn.py --k 128 --out r25_k128.json

--only-batch runs svdf_rank_topn (first top_n of --top) and svdf_rank_eval_positions (3 positives per section, the same bans) --reps times
each after a warm-up: the program to put behind `rocprofv3 --kernel-trace --stats --` in a run of its own.  k_rank_topn_sweep and
k_rank_eval_sweep score the same candidates with the same loop, so the ratio of their times is the price of the selection."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rank_eval import item_lines, sections   # noqa: E402


def tag_lines(users, pick_ban):
    """USER, BAN_SAMPLE, PROCESS per section as one CSRData (ids travel in the user field)"""
    import svdfeature_amd as sa
    S = len(users)
    idx = np.concatenate([users[:, None], pick_ban.reshape(S, 100)], axis=1).astype(np.uint32)
    base = 101 * np.arange(S, dtype=np.int64)[:, None]
    rp = np.concatenate([base + o for o in ([0, 0, 1], [1, 1, 101], [101, 101, 101])], axis=1)   # (g, u, i) starts of the 3 rows
    row_ptr = np.concatenate([rp.ravel(), [101 * S]]).astype(np.int32)
    label = np.tile(np.array([2.0, -1.0, 4.0], np.float32), S)
    return sa.CSRData(label, row_ptr, idx.ravel(), np.ones(idx.size, np.float32))


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
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
    tops = [int(x) for x in a.top.split(",")]
    t = sa.Trainer(0, 3)
    t.seed(7)
    for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(1000000, nu, ni, seed=3)))
    t.synchronize()
    users, pos_ptr, pos_item, ban_ptr, ban_item = sections(S, nu, ni, seed=11)
    rec = {"k": k, "sections": S, "items": ni, "banned": 100, "reps": a.reps, "top": {}}
    ok = True
    if a.only_batch:
        N = tops[0]
        t.rank_topn(users, N, ban_ptr, ban_item)
        t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)
        topn_s, eval_s = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            t.rank_topn(users, N, ban_ptr, ban_item)
            topn_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)
            eval_s.append(time.perf_counter() - t0)
        rec["top"][str(N)] = {"batch_s": spread(topn_s), "rank_eval_positions_s": spread(eval_s)}
    else:
        lines = tag_lines(users, ban_item)
        items_csr = item_lines(ni)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "m.model")
            t0 = time.perf_counter()
            t.save_model(path)
            rec["save_s"] = time.perf_counter() - t0
            rec["model_bytes"] = os.path.getsize(path)
            for N in tops:
                t0 = time.perf_counter()
                r = sa.Ranker(0, 3)
                r.set_param("top_k", str(N))
                r.load_model(path)
                r.init_ranker(ni)
                r.process_rows(items_csr)
                load_s = time.perf_counter() - t0
                more = t.rank_topn(users, N + 1, ban_ptr, ban_item)     # which sections have no tie among their N + 1 best (not timed)
                untied = (np.diff(more[1], axis=1) < 0).all(axis=1) & (more[2] == N + 1)
                got = t.rank_topn(users, N, ban_ptr, ban_item)          # warm-up: buffers, code objects
                want = r.process_rows(lines)                            # warm-up of the same kind
                batch_s, ranker_s = [], []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    got = t.rank_topn(users, N, ban_ptr, ban_item)
                    batch_s.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    want = r.process_rows(lines)
                    ranker_s.append(time.perf_counter() - t0)
                want = np.asarray(want).reshape(S, N)
                equal = bool(np.array_equal(got[0][untied], want[untied]))
                ok = ok and equal
                rec["top"][str(N)] = {"load_and_prepare_s": load_s, "batch_s": spread(batch_s), "ranker_s": spread(ranker_s),
                                      "speedup_median": float(np.median(ranker_s) / np.median(batch_s)),
                                      "sections_compared": int(untied.sum()), "sections_tied": int((~untied).sum()), "lists_equal": equal,
                                      "lists_equal_on_tied_sections_too": bool(np.array_equal(got[0], want)),
                                      "nan_sections": int(got[3].sum()), "ranker_tiles": r.counter(3), "ranker_host_sorts": r.counter(1)}
                r.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_topn: the batch call and the ranker disagree on a section without a tie")


if __name__ == "__main__":
    main()

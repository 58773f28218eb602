#!/usr/bin/env python3
"""Live-model ranking for sections with USER lines on a trainer with side tables (svdf_rank_topn_lines / svdf_rank_eval_positions_lines,
DESIGN.md section 6z) against the only route the parent had to the same answers: save the model, load it into sa.Ranker with the tables
set, push every section through process_rows (USER / POS_SAMPLE / BAN_SAMPLE / PROCESS lines).  Results in profiles/r30_rank_lines.md.

Input: tools/rank_eval.py's shape -- --sections sections (10 000) against --items items (100 000), 3 positives and 100 banned items per
section -- on a format_type = 0 model with feature_user and feature_item tables of --children (2) children per id, USER lines of
--line-len ids (1 or 4; the first with value 1, the others with values in (0.1, 1)), at one num_factor per invocation; the model has been
trained by one pass of rank pairs with the tables set.  The ranker route runs with top_k 0 (positions), 10 and 100.  The two routes
alternate --reps times (5) after a warm-up of each; medians with min .. max.  The answers of both routes are compared in the same run:
positions where the batch call reports no tie, lists on the sections whose top_n + 1 best scores are strictly decreasing.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 400 python tools/rank_lines.py --k 64 --line-len 1 --out r30_k64_l1.json && timeout -k 10 400 python tools/rank_lines.py --k 64 --line-len 4 --out r30_k64_l4.json

--only-batch runs the _lines calls alone (top_n of the first entry of --top, then the positions; --reps times each after a warm-up): the
program to put behind `rocprofv3 --kernel-trace --stats --` in a run of its own -- the times of k_rank_live_items and k_rank_live_rows
and their share of the call are in that trace.  The old calls on a plain model, parent build against this build, are
tools/rank_feedback.py --plain [--tree PARENT], alternating."""
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
from rank_feedback import spread, timed      # noqa: E402


def write_table(path, num_ids, children, seed):
    """`children` children per id, drawn from the whole id space, values in (0.1, 1)"""
    rng = np.random.default_rng(seed)
    idx, val = rng.integers(0, num_ids, (num_ids, children)), rng.uniform(0.1, 1.0, (num_ids, children)).astype(np.float32)
    with open(path, "w") as f:
        for i in range(num_ids):
            f.write("%d %s\n" % (children, " ".join("%d:%.9g" % (idx[i, c], val[i, c]) for c in range(children))))


def user_lines(users, nu, n, seed):
    """the section's user with value 1, then n - 1 attribute ids with values in (0.1, 1)"""
    rng = np.random.default_rng(seed)
    S = len(users)
    idx = np.concatenate([users[:, None], rng.integers(0, nu, (S, n - 1))], axis=1).astype(np.uint32)
    val = np.concatenate([np.ones((S, 1)), rng.uniform(0.1, 1.0, (S, n - 1))], axis=1).astype(np.float32)
    return (n * np.arange(S + 1)).astype(np.int64), idx.ravel(), val.ravel()


def tag_lines(sa, lines, n, pick_pos, pick_ban, with_pos):
    """USER, [POS_SAMPLE,] BAN_SAMPLE, PROCESS per section as one CSRData (ids travel in the user field)"""
    S = len(lines[0]) - 1
    parts, vals, sizes = [lines[1].reshape(S, n)], [lines[2].reshape(S, n)], [n]
    if with_pos:
        parts.append(pick_pos.reshape(S, 3))
        sizes.append(3)
    parts.append(pick_ban.reshape(S, 100))
    sizes += [100, 0]
    vals += [np.ones((S, sum(sizes) - n), np.float32)]
    idx = np.concatenate(parts, axis=1).astype(np.uint32)
    per = idx.shape[1]
    base = per * np.arange(S, dtype=np.int64)[:, None]
    ends = np.cumsum(sizes)
    rp = np.concatenate([base + np.array([e - z, e - z, e])[None, :] for e, z in zip(ends, sizes)], axis=1)   # (g, u, i) starts of each row
    row_ptr = np.concatenate([rp.ravel(), [per * S]]).astype(np.int32)
    label = np.tile(np.array(([2.0, 1.0] if with_pos else [2.0]) + [-1.0, 4.0], np.float32), S)
    return sa.CSRData(label, row_ptr, idx.ravel(), np.concatenate(vals, axis=1).ravel().astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
    ap.add_argument("--sections", type=int, default=10000)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--children", type=int, default=2)
    ap.add_argument("--line-len", type=int, default=1)
    ap.add_argument("--train-pairs", type=int, default=200000)
    ap.add_argument("--ranker-sections", type=int, default=0, help="sections the ranker route is timed on (0: all)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    nu, ni, S, k, L = a.users, a.items, a.sections, a.k, a.line_len
    tops = [int(x) for x in a.top.split(",")]
    users, pos_ptr, pos_item, ban_ptr, ban_item = sections(S, nu, ni, seed=11)
    lines = user_lines(users, nu, L, seed=12)
    rec = {"k": k, "sections": S, "items": ni, "positives": 3, "banned": 100, "children": a.children, "line_len": L, "reps": a.reps, "top": {}}
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        fu, fi = os.path.join(tmp, "feat_user.txt"), os.path.join(tmp, "feat_item.txt")
        write_table(fu, nu, a.children, 21)
        write_table(fi, ni, a.children, 22)
        tables = [("feature_user", fu), ("feature_item", fi)]
        t = sa.Trainer(0, 3)
        t.seed(7)
        for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05) + tables:
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        if a.train_pairs:
            t.update_batch(sa.pairs_as_csr(*cases.planted_pairs(a.train_pairs, nu, ni, seed=3)))
        t.synchronize()
        topn = lambda N: t.rank_topn(None, N, ban_ptr, ban_item, lines=lines)
        positions = lambda: t.rank_positions(None, pos_ptr, pos_item, ban_ptr, ban_item, lines=lines)
        if a.only_batch:
            topn(tops[0])
            positions()
            rec["top"][str(tops[0])] = {"batch_s": spread([timed(lambda: topn(tops[0]))[1] for _ in range(a.reps)])}
            rec["positions"] = {"batch_s": spread([timed(positions)[1] for _ in range(a.reps)])}
        else:
            R = a.ranker_sections or S
            rec["ranker_sections"] = R
            sub = (lines[0][:R + 1], lines[1][:L * R], lines[2][:L * R])
            path = os.path.join(tmp, "m.model")
            _, rec["save_s"] = timed(lambda: t.save_model(path))
            rec["model_bytes"] = os.path.getsize(path)
            items_csr = item_lines(ni)
            for N in [0] + tops:                        # 0: the positions
                def load():
                    r = sa.Ranker(0, 0)
                    for kk, v in tables + [("top_k", str(N))]:
                        r.set_param(kk, v)
                    r.load_model(path)
                    r.init_ranker(ni)
                    r.process_rows(items_csr)
                    return r
                r, load_s = timed(load)
                stream = tag_lines(sa, sub, L, pos_item[:3 * R], ban_item[:100 * R], N == 0)
                ranker = lambda: r.process_rows(stream)
                batch = positions if N == 0 else (lambda: topn(N))
                got, want = batch(), ranker()           # warm-up of each
                batch_s, ranker_s = [], []
                for _ in range(a.reps):
                    got, dt = timed(batch)
                    batch_s.append(dt)
                    want, dt = timed(ranker)
                    ranker_s.append(dt)
                bm, rm = spread(batch_s), spread(ranker_s)
                e = {"load_and_prepare_s": load_s, "batch_s": bm, "ranker_s": rm, "ranker_s_per_section": rm["median"] / R,
                     "batch_s_per_section": bm["median"] / S, "ratio_per_section": rm["median"] / R / (bm["median"] / S),
                     "beats_by_more_than_both_spreads": bool(rm["min"] / R > bm["max"] / S), "nan_sections": int(got[3].sum())}
                want = np.asarray(want)
                if N == 0:
                    n = int(pos_ptr[R])
                    untied = got[1][:n] == 0
                    e.update(compared=int(untied.sum()), tied=int((~untied).sum()), equal=bool(np.array_equal(got[0][:n][untied], want[untied])))
                    rec["positions"] = e
                else:
                    more = topn(N + 1)
                    untied = ((np.diff(more[1], axis=1) < 0).all(axis=1) & (more[2] == N + 1))[:R]
                    e.update(compared=int(untied.sum()), tied=int((~untied).sum()), equal=bool(np.array_equal(got[0][:R][untied], want.reshape(R, N)[untied])))
                    rec["top"][str(N)] = e
                ok = ok and e["equal"]
                r.close()
        rec["counter_41"] = t.counter(41)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_lines: the batch call and the ranker disagree where nothing ties")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Live-model ranking for user-group (SVD++) trainers (svdf_rank_topn_fb / svdf_rank_eval_positions_fb) against the route
the parent had to the same answers: save the model, load it into sa.Ranker(1, 0), push every section through process_block (its feedback
list; USER / POS_SAMPLE / BAN_SAMPLE / PROCESS lines).  Results in profiles/r29_rank_feedback.md.

Input: tools/rank_eval.py's shape on a user-group model -- --sections sections (10 000) against --items items (100 000), num_ufeedback =
--feedback (100 000), --fb-len feedback entries (100), 100 banned items and 3 positives per section, at one num_factor per invocation; the
model has been trained by one pass of --train-blocks SVD++ user blocks.  The ranker has no batch call for blocks: a section costs it the
same whichever sections surround it, so it is timed on the first --ranker-sections sections (all of them by default) and its time is also
given per section.  The two routes alternate --reps times (5) after a warm-up of each; medians with min .. max.  The answers of both routes
are compared in the same run: positions where the batch call reports no tie, lists on the sections whose top_n + 1 best scores are
strictly decreasing.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 400 python tools/rank_feedback.py --k 64 --out r29_k64.json && timeout -k 10 400 python tools/rank_feedback.py --k 128 --out r29_k128.json

--only-batch runs the _fb calls alone (first top_n of --top, then the positions; --reps times each after a warm-up): the program to put
behind `rocprofv3 --kernel-trace --stats --` in a run of its own -- k_rank_live_rows' time and its share of the call are in that trace.
--plain runs the OLD calls (rank_topn, rank_positions) on the format_type = 0 model of tools/rank_topn.py instead: the same command on two
builds, alternating, is the measurement that the sweeps have not slowed (--tree names the checkout whose built svdfeature_amd package is
imported instead of this one's)."""
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


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def feedback_lists(S, nfb, n, seed):
    """n distinct feedback ids per section with the demo's value n^-1/2 (mkimplicitfeedbackfeature.py:46-55)"""
    rng = np.random.default_rng(seed)
    offs = rng.choice(nfb, n, replace=False)
    idx = ((rng.integers(0, nfb, S)[:, None] + offs[None, :]) % nfb).astype(np.uint32)
    return (n * np.arange(S + 1)).astype(np.int64), idx.ravel(), np.full(S * n, 1.0 / np.sqrt(n), np.float32)


def section_block(sa, user, fb_idx, fb_val, pos, ban):
    rows = [(2.0, [], [(int(user), 1.0)], [])]
    if pos is not None:
        rows.append((1.0, [], [(int(x), 1.0) for x in pos], []))
    rows.append((-1.0, [], [(int(x), 1.0) for x in ban], []))
    rows.append((4.0, [], [], []))
    return sa.PlusBlock(fb_idx, fb_val, sa.CSRData.from_rows(rows), 0)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="10,100")
    ap.add_argument("--sections", type=int, default=10000)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--feedback", type=int, default=100000)
    ap.add_argument("--fb-len", type=int, default=100)
    ap.add_argument("--train-blocks", type=int, default=3000)
    ap.add_argument("--ranker-sections", type=int, default=0, help="sections the ranker route is timed on (0: all)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--tree", default=None, help="another built checkout of the project: its svdfeature_amd package is imported instead of this tree's")
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    if a.tree:
        sys.path.insert(0, os.path.abspath(a.tree))
    import cases
    import svdfeature_amd as sa
    nu, ni, S, k, nfb = a.users, a.items, a.sections, a.k, a.feedback
    tops = [int(x) for x in a.top.split(",")]
    users, pos_ptr, pos_item, ban_ptr, ban_item = sections(S, nu, ni, seed=11)
    rec = {"k": k, "sections": S, "items": ni, "positives": 3, "banned": 100, "reps": a.reps, "tree": a.tree or "."}
    ok = True
    if a.plain:
        t = sa.Trainer(0, 3)
        t.seed(7)
        for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(1000000, nu, ni, seed=3)))
        t.synchronize()
        rec["plain"] = {}
        for N in tops:
            t.rank_topn(users, N, ban_ptr, ban_item)
            rec["plain"]["topn_%d_s" % N] = spread([timed(lambda: t.rank_topn(users, N, ban_ptr, ban_item))[1] for _ in range(a.reps)])
        t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)
        rec["plain"]["positions_s"] = spread([timed(lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item))[1] for _ in range(a.reps)])
    else:
        t = sa.Trainer(1, 0)
        t.seed(7)
        for kk, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05, num_ufeedback=nfb,
                                     wd_ufeedback=0.004, ufeedback_init_sigma=0.05):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        for b in cases.user_blocks(a.train_blocks, nu, ni, nfb, seed=3, max_fb=20):
            t.update_block(b)
        t.synchronize()
        fb = feedback_lists(S, nfb, a.fb_len, seed=12)
        rec.update(feedback=nfb, fb_len=a.fb_len, top={})
        topn = lambda N: t.rank_topn(users, N, ban_ptr, ban_item, feedback=fb)
        positions = lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item, feedback=fb)
        if a.only_batch:
            topn(tops[0])
            positions()
            rec["top"][str(tops[0])] = {"batch_s": spread([timed(lambda: topn(tops[0]))[1] for _ in range(a.reps)])}
            rec["positions"] = {"batch_s": spread([timed(positions)[1] for _ in range(a.reps)])}
        else:
            R = a.ranker_sections or S
            rec["ranker_sections"] = R
            fbp, fbi, fbv = fb
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "m.model")
                _, rec["save_s"] = timed(lambda: t.save_model(path))
                rec["model_bytes"] = os.path.getsize(path)
                items_csr = item_lines(ni)
                for N in [0] + tops:                        # 0: the positions
                    def load():
                        r = sa.Ranker(1, 0)
                        r.set_param("top_k", str(N))
                        r.load_model(path)
                        r.init_ranker(ni)
                        r.process_rows(items_csr)
                        return r
                    r, load_s = timed(load)
                    blocks = [section_block(sa, users[s], fbi[fbp[s]:fbp[s + 1]], fbv[fbp[s]:fbp[s + 1]],
                                            pos_item[pos_ptr[s]:pos_ptr[s + 1]] if N == 0 else None, ban_item[ban_ptr[s]:ban_ptr[s + 1]]) for s in range(R)]
                    ranker = lambda: np.concatenate([r.process_block(b) for b in blocks])
                    batch = positions if N == 0 else (lambda: topn(N))
                    got, want = batch(), ranker()           # warm-up of each
                    batch_s, ranker_s = [], []
                    for _ in range(a.reps):
                        got, dt = timed(batch)
                        batch_s.append(dt)
                        want, dt = timed(ranker)
                        ranker_s.append(dt)
                    e = {"load_and_prepare_s": load_s, "batch_s": spread(batch_s), "ranker_s": spread(ranker_s),
                         "ranker_s_per_section": float(np.median(ranker_s)) / R, "batch_s_per_section": float(np.median(batch_s)) / S,
                         "ratio_per_section": float(np.median(ranker_s)) / R / (float(np.median(batch_s)) / S), "nan_sections": int(got[3].sum())}
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
        rec["counter_40"] = t.counter(40)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_feedback: the batch call and the ranker disagree where nothing ties")


if __name__ == "__main__":
    main()

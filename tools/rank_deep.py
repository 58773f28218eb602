#!/usr/bin/env python3
"""Deep top-N lists on the live model (knob rank_topn_deep = 1, top_n 257 .. 4096) against the only route the parent
had to the same lists: save the model, load it into a svdf_ranker with top_k set, feed every user as tag lines (sa.Ranker.process_rows).
Results in profiles/r46_rank_deep.md.

Input: tools/rank_topn.py's -- --sections users (10 000) against --items items (100 000) at one num_factor per invocation, 100 banned items
per section, the model trained by one pass of rank pairs first.  For every top_n of --top (500,1000,4096): the ranker's save and load (+ the
candidate matrix) are timed once; then the three routes -- the ranker, the deep call with rank_topn_scores 0 (pinned) and 1 (matrix) --
alternate --reps times (5) on the same sections after a warm-up of each; medians with min .. max of the host clock around the call, which
ends in a synchronise.  Cuts per list: no kernel counts them; the sweeps' list rule is walked on the host for --cuts seeded sections (32)
over float32 numpy scores of the live model, at the pinned sweep's step and the call's geometry (--only-cuts: that alone).  The pinned lists
are compared with the ranker's on every section whose listed scores are strictly decreasing and whose last listed item ties with no
unlisted candidate (svdf_rank_eval_positions reports that, in the same pinned scores); how many sections are tied is reported.
--no-ranker leaves the ranker route out.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 400 python tools/rank_deep.py --k 64 --out r46_k64.json && timeout -k 10 400 python tools/rank_deep.py --k 128 --out r46_k128.json

--only-batch runs the deep call (first top_n of --top, mode --scores) and the knob-0 call at top_n 256 --reps times each after a warm-up:
the program to put behind `rocprofv3 --kernel-trace --stats --` in a run of its own.  Both sweeps score the same candidates with the same
loop, so the difference of their times is what the deeper selection costs; k_rank_topn_merge_deep against k_rank_topn_merge likewise."""
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
from rank_topn import spread, tag_lines      # noqa: E402

def emulated_cuts(score, on, per, step, top_n, cap):
    """the sweeps' list rule (append what beats the threshold, cut a list that cannot take a whole step to its top_n largest) walked on
    the host over one section's scores: how often each of its lists is cut.  Keys are ranks in the (score, -id) order, so they are distinct."""
    ni = len(score)
    rank = np.empty(ni, np.int64)
    rank[np.lexsort((-np.arange(ni), score))] = np.arange(ni)
    cuts = []
    for y0 in range(0, ni, per):
        kept, thr, c, y1 = np.empty(0, np.int64), -1, 0, min(y0 + per, ni)
        for s0 in range(y0, y1, step):
            if len(kept) + step > cap:
                kept = np.sort(kept)[-top_n:]
                thr, c = kept[0], c + 1
            r = rank[s0:min(s0 + step, y1)]
            kept = np.concatenate([kept, r[on[s0:s0 + len(r)] & (r > thr)]])
        cuts.append(c)
    return cuts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--top", default="500,1000,4096")
    ap.add_argument("--sections", type=int, default=10000)
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--users", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scores", type=int, default=0, help="--only-batch: the scoring mode of the deep call")
    ap.add_argument("--only-batch", action="store_true")
    ap.add_argument("--no-ranker", action="store_true")
    ap.add_argument("--cuts", type=int, default=32, help="sections the cuts per list are emulated for (pinned mode's step)")
    ap.add_argument("--only-cuts", action="store_true", help="no timings: the geometry and the emulated cuts alone")
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
    users, _, _, ban_ptr, ban_item = sections(S, nu, ni, seed=11)

    def deep(N, scores):
        t.set_knob("rank_topn_deep", 1)
        t.set_knob("rank_topn_scores", scores)
        return t.rank_topn(users, N, ban_ptr, ban_item)

    def flat():
        t.set_knob("rank_topn_deep", 0)
        t.set_knob("rank_topn_scores", a.scores)
        return t.rank_topn(users, 256, ban_ptr, ban_item)

    def timed(routes):
        """the routes alternate a.reps times after a warm-up of each; returns ({route: last result}, {route: spread})"""
        got = {r: f() for r, f in routes.items()}
        secs = {r: [] for r in routes}
        for _ in range(a.reps):
            for r, f in routes.items():
                t0 = time.perf_counter()
                got[r] = f()
                secs[r].append(time.perf_counter() - t0)
        return got, {r: spread(x) for r, x in secs.items()}

    def cuts(N):
        """cuts per list of the pinned deep sweep, emulated for a.cuts seeded sections on float32 numpy scores of the live model"""
        t.set_knob("rank_topn_deep", 1)
        t.set_knob("rank_topn_scores", 0)
        g = t.rank_geometry("topn", S, N)
        U, W, bias = t.view("W_user"), t.view("W_item"), t.view("i_bias")
        step, all_cuts = 128 if k <= 128 else 64, []
        for s in np.random.default_rng(5).permutation(S)[:a.cuts]:
            on = np.ones(ni, bool)
            on[ban_item[ban_ptr[s]:ban_ptr[s + 1]].astype(np.int64)] = False
            all_cuts += emulated_cuts(bias + W @ U[users[s]], on, g["items_per_block"], step, N, g["cap"])
        return {"cap": g["cap"], "gy": g["gy"], "pieces": -(-S // g["sections"]), "items_per_range": g["items_per_block"],
                "cuts_per_list": {"mean": float(np.mean(all_cuts)), "min": int(min(all_cuts)), "max": int(max(all_cuts)), "lists": len(all_cuts)}}

    rec = {"k": k, "sections": S, "items": ni, "banned": 100, "reps": a.reps, "top": {}}
    ok = True
    if a.only_cuts:
        rec["top"] = {str(N): cuts(N) for N in tops}
    elif a.only_batch:
        N = tops[0]
        _, secs = timed({"top256": flat, "deep": lambda: deep(N, a.scores)})   # (the deep call last: the probe below answers under its knobs)
        rec["top"][str(N)] = dict(secs, scores=a.scores, pieces=-(-S // t.rank_geometry("topn", S, N)["sections"]))
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "m.model")
            lines = items_csr = None
            if not a.no_ranker:
                lines, items_csr = tag_lines(users, ban_item), item_lines(ni)
                t0 = time.perf_counter()
                t.save_model(path)
                rec["save_s"] = time.perf_counter() - t0
            for N in tops:
                routes = {"pinned": lambda: deep(N, 0), "matrix": lambda: deep(N, 1)}
                run = {}
                if not a.no_ranker:
                    t0 = time.perf_counter()
                    r = sa.Ranker(0, 3)
                    r.set_param("top_k", str(N))
                    r.load_model(path)
                    r.init_ranker(ni)
                    r.process_rows(items_csr)
                    run["load_and_prepare_s"] = time.perf_counter() - t0
                    routes["ranker"] = lambda: r.process_rows(lines)
                got, secs = timed(routes)
                run.update(cuts(N))
                run.update({"nan_sections": int(got["pinned"][3].sum()),
                            "matrix_same_ids": float((got["pinned"][0] == got["matrix"][0]).mean())})
                run.update({name + "_s": s for name, s in secs.items()})
                if not a.no_ranker:
                    # which sections have no tie among the scores listed, nor between the last one and an unlisted candidate (not timed):
                    # the positions call reports, in the same pinned scores, how many ranked candidates tie with a section's last listed item
                    mine = got["pinned"]
                    full = mine[2] == N
                    last = np.where(full, mine[0][:, N - 1], 0).astype(np.uint32)
                    tied = t.rank_positions(users, np.arange(S + 1, dtype=np.int64), last, ban_ptr, ban_item)[1]
                    untied = (np.diff(mine[1], axis=1) < 0).all(axis=1) & full & (tied == 0)
                    want = np.asarray(got["ranker"]).reshape(S, N)
                    equal = bool(np.array_equal(mine[0][untied], want[untied]))
                    ok = ok and equal
                    run.update({"sections_compared": int(untied.sum()), "sections_tied": int((~untied).sum()), "lists_equal": equal,
                                "lists_differing_on_tied_sections": int((got["pinned"][0] != want).any(axis=1)[~untied].sum()),
                                "ranker_over_pinned": secs["ranker"]["median"] / secs["pinned"]["median"],
                                "ranker_over_matrix": secs["ranker"]["median"] / secs["matrix"]["median"]})
                    r.close()
                rec["top"][str(N)] = run
    t.set_knob("rank_topn_deep", 0)
    t.set_knob("rank_topn_scores", 0)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_deep: the deep call and the ranker disagree on a section without a tie")


if __name__ == "__main__":
    main()

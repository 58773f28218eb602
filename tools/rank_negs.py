#!/usr/bin/env python3
"""Live-model ranking against negatives drawn on the device (svdf_rank_eval_positions_sampled).
Results in profiles/r32_rank_negs.md.

Input: tools/rank_cand.py's format_type = 0 pair model of --users x --items at one num_factor per invocation; --sections sections (users
drawn with replacement), each with one positive and --bans distinct banned ids (one random set of offsets rotated by a per-section base).

--mode same      (2 000 sections x 20 000 items) and
--mode workload  (10 000 sections x 100 000 items): the sampled call against the only route the parent had to the same answers -- the same
                 negatives from svdf_rank_negatives on the host (timed separately) handed to rank_positions(candidates=).  The two routes
                 alternate --reps times (5) after a warm-up of each; medians with min .. max; every output of both routes is compared in
                 the same run; the upload of each route per call is counted in bytes from the sizes of its tables.
--mode kernel    the sampled call alone: the program to put behind `rocprofv3 --kernel-trace --stats --` in a run of its own, for the draw
                 kernel's own time.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_negs.py --mode workload --k 64 --out r32_k64.json && timeout -k 10 300 python tools/rank_negs.py --mode workload --k 128 --out r32_k128.json

The old calls on a plain model, parent build against this build, are tools/rank_feedback.py --plain [--tree PARENT], alternating."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rank_feedback import spread, timed      # noqa: E402

SHAPES = {"same": (2000, 20000, 20000), "workload": (10000, 100000, 20000), "kernel": (10000, 100000, 20000)}   # sections, items, users


def lists(S, nu, ni, B, seed):
    """(users, pos_ptr, pos_item, ban_ptr, ban_item): one positive and B distinct bans per section, none of them the positive"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    offs = rng.choice(ni, B + 1, replace=False)
    pick = ((rng.integers(0, ni, S)[:, None] + offs[None, :]) % ni).astype(np.uint32)
    return users, np.arange(S + 1, dtype=np.int64), np.ascontiguousarray(pick[:, 0]), (B * np.arange(S + 1)).astype(np.int64), np.ascontiguousarray(pick[:, 1:]).ravel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=sorted(SHAPES), default="workload")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--num-neg", default="99,999")
    ap.add_argument("--bans", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--sections", type=int, default=0)
    ap.add_argument("--items", type=int, default=0)
    ap.add_argument("--users", type=int, default=0)
    ap.add_argument("--train-pairs", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    S, ni, nu = (x or d for x, d in zip((a.sections, a.items, a.users), SHAPES[a.mode]))
    k = a.k
    pitch = (k + 3) // 4 * 4
    t = sa.Trainer(0, 3)
    t.seed(7)
    for kk, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.05):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    if a.train_pairs:
        t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(a.train_pairs, nu, ni, seed=3)))
    t.synchronize()
    users, pos_ptr, pos_item, ban_ptr, ban_item = lists(S, nu, ni, a.bans, seed=11)
    rec = {"mode": a.mode, "k": k, "pitch": pitch, "sections": S, "items": ni, "bans": a.bans, "reps": a.reps, "negs": {}}
    ok = True
    for M in [int(x) for x in a.num_neg.split(",")]:
        new = lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item, sampled=(M, a.seed))
        new_neg = lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item, sampled=(M, a.seed), return_negatives=True)
        pairs = S * (M + 1)
        ntile = S * ((M + 1 + 63) // 64)
        # words of a piece's one upload (svdf_ranknegs.cpp / svdf_rankcand.cpp), 4 bytes each; cand_id is a device workspace in the sampled route
        e = {"pairs": pairs, "gather_bytes": pairs * pitch * 4,
             "sampled_upload_bytes": 4 * (S + 3 * (S + 1) + 2 * ntile + 1 + 2 * S + S * (a.bans + 1)),
             "cand_upload_bytes": 4 * (S + 2 * (S + 1) + pairs + 2 * ntile + 1 + S)}
        if a.mode == "kernel":
            new()
            e["sampled_s"] = spread([timed(new)[1] for _ in range(a.reps)])
        else:
            draw = lambda: sa.rank_negatives(ni, pos_ptr, pos_item, ban_ptr, ban_item, M, a.seed)
            neg = draw()
            e["host_draw_s"] = spread([timed(draw)[1] for _ in range(a.reps)])
            cand = (M * np.arange(S + 1, dtype=np.int64), neg.astype(np.uint32).ravel())
            old = lambda: t.rank_positions(users, pos_ptr, pos_item, candidates=cand)
            got, want = new_neg(), old()           # warm-up of each
            ok = ok and bool(np.array_equal(got[4], neg))
            new_s, old_s, neg_s = [], [], []
            for _ in range(a.reps):
                got, dt = timed(new)
                new_s.append(dt)
                want, dt = timed(old)
                old_s.append(dt)
                _, dt = timed(new_neg)
                neg_s.append(dt)
            nm, om = spread(new_s), spread(old_s)
            e.update({"sampled_s": nm, "sampled_with_negatives_s": spread(neg_s), "cand_s": om, "ratio_cand_over_sampled": om["median"] / nm["median"],
                      "beats_by_more_than_both_spreads": bool(om["min"] > nm["max"]),
                      "equal": bool(all(np.array_equal(x, y) for x, y in zip(got, want)))})
            ok = ok and e["equal"]
        rec["negs"][str(M)] = e
    rec["counter_43"] = t.counter(43)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_negs: the sampled call and the candidate call on the same negatives disagree")


if __name__ == "__main__":
    main()

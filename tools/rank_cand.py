#!/usr/bin/env python3
"""Live-model ranking over per-section candidate lists (svdf_rank_eval_positions_cand / svdf_rank_topn_cand).
Results in profiles/r31_rank_cand.md.

Input: a format_type = 0 pair model (tools/rank_topn.py's) of --users x --items at one num_factor per invocation, trained by one pass of
rank pairs; --sections sections (users drawn with replacement), each with a candidate list of --list-len DISTINCT ids (one random set of
offsets rotated by a per-section base, as tools/rank_eval.py draws its lists), the first of which is the section's one positive.

--mode same      (2 000 sections x 20 000 items): the new calls against the only route the parent had to the same answers, the old calls
                 given the complement of each list as bans.  Positions and top-10; the two routes alternate --reps times (5) after a
                 warm-up of each; medians with min .. max; every output of both routes is compared in the same run.
--mode workload  (10 000 sections x 100 000 items): the new calls alone, the time per call and the bytes/s of the gather per call, counting
                 pairs x pitch x 4; beside them the full-catalogue call on the same sections (no bans) -- a DIFFERENT answer, for scale.
--mode kernel    the new top-10 call alone with the score kernel's form forced by --form (1 one lane per pair, 2 staged): the program to
                 put behind `rocprofv3 --kernel-trace --stats --` in a run of its own.

One invocation is one GPU step; run each under its own time limit and chain them:

    timeout -k 10 300 python tools/rank_cand.py --mode same --k 64 --out r31_same_k64.json && timeout -k 10 300 python tools/rank_cand.py --mode same --k 128 --out r31_same_k128.json

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


def lists(S, nu, ni, L, seed):
    """(users, pos_ptr, pos_item, cand_ptr, cand_item): L distinct ids per section, the first of them its positive"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    offs = rng.choice(ni, L, replace=False)
    pick = ((rng.integers(0, ni, S)[:, None] + offs[None, :]) % ni).astype(np.uint32)
    return users, np.arange(S + 1, dtype=np.int64), np.ascontiguousarray(pick[:, 0]), (L * np.arange(S + 1)).astype(np.int64), pick.ravel()


def complement(S, ni, L, cand_item):
    """per section every id that is not in its list, ascending: the bans under which the old calls rank the same sets"""
    on = np.ones((S, ni), bool)
    on[np.repeat(np.arange(S), L), cand_item] = False
    return ((ni - L) * np.arange(S + 1)).astype(np.int64), np.nonzero(on)[1].astype(np.uint32)


def same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x, np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
               for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=sorted(SHAPES), default="same")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--list-len", default="100,1000")
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--sections", type=int, default=0)
    ap.add_argument("--items", type=int, default=0)
    ap.add_argument("--users", type=int, default=0)
    ap.add_argument("--train-pairs", type=int, default=200000)
    ap.add_argument("--form", type=int, default=0, help="knob rank_cand_form: 0 the measured choice, 1 one lane per pair, 2 staged")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="file the JSON record is also written to")
    a = ap.parse_args()
    import cases
    import svdfeature_amd as sa
    S, ni, nu = (x or d for x, d in zip((a.sections, a.items, a.users), SHAPES[a.mode]))
    k, N = a.k, a.top
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
    t.set_knob("rank_cand_form", a.form)
    rec = {"mode": a.mode, "k": k, "pitch": pitch, "sections": S, "items": ni, "top_n": N, "form": a.form, "reps": a.reps, "lists": {}}
    ok = True
    for L in [int(x) for x in a.list_len.split(",")]:
        users, pos_ptr, pos_item, cand_ptr, cand_item = lists(S, nu, ni, L, seed=11 + L)
        cand = (cand_ptr, cand_item)
        new_pos = lambda: t.rank_positions(users, pos_ptr, pos_item, candidates=cand)
        new_top = lambda: t.rank_topn(users, N, candidates=cand)
        e = {"pairs": S * L, "gather_bytes": S * L * pitch * 4}
        if a.mode == "kernel":
            new_top()
            e["topn_s"] = spread([timed(new_top)[1] for _ in range(a.reps)])
        elif a.mode == "workload":
            for name, call in (("positions", new_pos), ("topn", new_top), ("full_catalogue_positions", lambda: t.rank_positions(users, pos_ptr, pos_item)),
                               ("full_catalogue_topn", lambda: t.rank_topn(users, N))):
                call()
                e[name + "_s"] = spread([timed(call)[1] for _ in range(a.reps)])
            for name in ("positions", "topn"):
                e[name + "_gather_bytes_per_s_of_the_call"] = e["gather_bytes"] / e[name + "_s"]["median"]
        else:
            ban_ptr, ban_item = complement(S, ni, L, cand_item)
            e["ban_entries"] = int(ban_ptr[-1])
            for name, new, old in (("positions", new_pos, lambda: t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)),
                                   ("topn", new_top, lambda: t.rank_topn(users, N, ban_ptr, ban_item))):
                got, want = new(), old()           # warm-up of each
                new_s, old_s = [], []
                for _ in range(a.reps):
                    got, dt = timed(new)
                    new_s.append(dt)
                    want, dt = timed(old)
                    old_s.append(dt)
                nm, om = spread(new_s), spread(old_s)
                e[name] = {"cand_s": nm, "complement_bans_s": om, "ratio": om["median"] / nm["median"],
                           "beats_by_more_than_both_spreads": bool(om["min"] > nm["max"]), "equal": bool(same(got, want))}
                ok = ok and e[name]["equal"]
        rec["lists"][str(L)] = e
    rec["counter_42"] = t.counter(42)
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("rank_cand: the candidate call and the old call under complement bans disagree")


if __name__ == "__main__":
    main()

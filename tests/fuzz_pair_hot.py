#!/usr/bin/env python3
"""(not collected by pytest) Randomised differential run of the ordered sub-steps for hot items of rank pairs in the window step (knob
`window_pair_sub`; svdf_wseq.cpp: wseq_from_pairs, svdf_k_window.hip: k_window_apply_pairs).  Random widths (the two
slots-walk widths drawn often), links, regularisers (per-id decay ranges on both sides, nonnegative users, user bias on and off, bias decays),
catalogue sizes, skew (0 ... 4 hot items, drawn as positive and as negative with random probabilities), window sizes, passes and a random
sub-step 1 ... 16 (1 ... 128 in one draw of eight): `amd:step = minibatch` on one GPU against the checker of tests/window_sim.py on the
pair-shaped rows, bit for bit.
usage: python tests/fuzz_pair_hot.py --iters 150 --seed 1"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cases
import fuzz_side_table
import pair_hot_cases as ph
import svdfeature_amd as sa


def one(rng):
    k = int(rng.choice([1, 3, 8, 16, 33, 64, 64, 100, 128, 128, 200, 256]))
    nu = int(rng.integers(5, 60))
    ni = int(rng.integers(3, 8)) if rng.random() < 0.4 else int(rng.integers(8, 60))
    n = int(rng.integers(20, 300))
    active = int(rng.choice([0, 2, 3, 3]))
    contract = k in (64, 128) and rng.random() < 0.5   # the slots walk: sigmoid rank loss, L2 decay, no user bias, no ranges
    reg = 0 if contract else int(rng.integers(0, 4))
    extra = {}
    if contract:
        active = 3
        extra["no_user_bias"] = "1"
    else:
        if rng.random() < 0.4: extra["no_user_bias"] = "1"
        if rng.random() < 0.3: extra["user_nonnegative"] = "1"
        if rng.random() < 0.3: extra["wd_user_bias"] = "0.01"
    if rng.random() < 0.4: extra["wd_item_bias"] = "0.02"
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=0, num_factor=k, reg_method=reg, active_type=active,
                           learning_rate=str(float(rng.choice([0.005, 0.01, 0.02]))), **extra)
    if active != 0:
        conf = cases.conf_with(conf, base_score="0.5")
    if not contract and rng.random() < 0.3:
        cut = int(rng.integers(1, nu + 1))
        conf += [("up:wd", "0.01"), ("up:bound", str(cut)), ("up:wd", "0.002"), ("up:bound", str(nu))]
    if not contract and rng.random() < 0.4:
        cut = int(rng.integers(1, ni))
        conf += [("ip:wd", "0.01"), ("ip:bound", str(cut)), ("ip:wd", "0.002"), ("ip:bound", str(ni))]
    hot = tuple(int(x) for x in rng.choice(ni, size=min(ni - 2, int(rng.integers(0, 5))), replace=False))
    u, p, q = ph.draw_pairs(rng, n, p_pos=float(rng.uniform(0, 0.9)), p_neg=float(rng.uniform(0, 0.9)), hot=hot, nu=nu, ni=ni)
    window = int(rng.integers(1, n + 1))
    s = int(rng.integers(1, 129)) if rng.random() < 0.125 else int(rng.integers(1, 17))
    return dict(k=k, nu=nu, ni=ni, active=active, reg=reg, extra=extra, conf=conf, u=u, p=p, q=q, window=window, passes=int(rng.integers(1, 4)), s=s)


def check(c):
    t = sa.Trainer(0, c["active"])
    t.seed(10)
    for kk, v in c["conf"] + [("amd:step", "minibatch"), ("amd:window", str(c["window"]))]:
        t.set_param(kk, str(v))
    t.init_model()
    t.init_trainer()
    t.set_knob("window_pair_sub", c["s"])
    ds = t.dataset_from_pairs(c["u"], c["p"], c["q"])
    for _ in range(c["passes"]):
        t.train_dataset(ds)
    t.synchronize()
    W = ds.num_batches
    o = ph.check(c["conf"], c["u"], c["p"], c["q"], W, c["passes"], c["s"])
    bad = [name for name in ph.VIEWS if not fuzz_side_table.same(t.view(name), o.view(name))]   # (bit for bit; a value both sides lost to NaN matches whatever its payload)
    f = ph.facts(c["p"], c["q"], W, c["s"])
    desc = dict(k=c["k"], nu=c["nu"], ni=c["ni"], n=len(c["u"]), active=c["active"], reg=c["reg"], extra=c["extra"], windows=W, passes=c["passes"],
                s=c["s"], hot_rows=f["nhot"], two_hot=int(f["two_hot"]), diverged=bool(any(np.isnan(o.view(name)).any() for name in ph.VIEWS)))
    ds.close(); t.close(); o.close()
    return bad, desc


def run(iters, seed, verbose=False):
    rng = np.random.default_rng(seed)
    fails = diverged = with_hot = hot_rows = two_hot = 0
    for it in range(iters):
        bad, desc = check(one(rng))
        diverged += desc["diverged"]
        with_hot += desc["hot_rows"] > 0
        hot_rows += desc["hot_rows"]
        two_hot += desc["two_hot"]
        if bad:
            fails += 1
            print(json.dumps({"iter": it, "mismatch": bad, **desc}), flush=True)
        elif verbose and it % 25 == 0:
            print("iter %d ok" % it, flush=True)
    print(json.dumps({"fuzz": "pair_hot", "iters": iters, "seed": seed, "mismatches": fails, "diverged": diverged,
                      "draws_with_hot_rows": with_hot, "hot_rows": hot_rows, "pairs_with_two_hot_items": two_hot}), flush=True)
    return fails


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run(a.iters, a.seed, verbose=True) else 0)

"""Checker of the window step with shared user rows (`amd:shared_user_from = B`, svdf_wunit.cpp / svdf_k_wunit.hip),
built on the pinned C port of the reference (oracle.OracleTrainer("port")), one window at a time:

  * snapshot of the shared state: W_item, i_bias, g_bias and the rows >= B of W_user / u_bias;
  * every row of the window, in file order: the shared parts are set back to the snapshot (private user rows keep their current values),
    the row is the reference's update_inner (update_csr), and new - snapshot of every target the row touches is added, in fp32 and in file
    order, to that target's accumulator (acc = +0 + c_1 + c_2 ...);
  * at the window's end every touched target becomes snapshot + acc.

Rows with one user entry and no shared ids make this the existing checker (oracle update_batch_stale + the window's add), which
tests/test_shared_user_checker.py pins bit for bit."""
import numpy as np

from oracle import oracle
from svdfeature_amd import CSRData

SHARED = ("W_item", "i_bias", "g_bias", "W_user", "u_bias")


def make_oracle(conf, seed=10, active=0):
    t = oracle.OracleTrainer("port", 0, active)
    t.seed(seed)
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    return t


def _views(o):
    return {name: o.view(name).copy() for name in SHARED}


def window_step(o, d, B, user_bias=True):
    """one window (CSRData d, rows in file order) on oracle trainer o; user ids >= B are shared rows"""
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in SHARED}
    cur = {name: v.copy() for name, v in snap.items()}
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        gids = [int(x) for x in idx[:ng]]
        uids = [int(x) for x in idx[ng:ng + nu]]
        iids = [int(x) for x in idx[ng + nu:]]
        shared = [u for u in uids if u >= B]
        # the shared parts as they were at the window start; private user rows as they are now
        cur["W_item"][...] = snap["W_item"]
        cur["i_bias"][...] = snap["i_bias"]
        cur["g_bias"][...] = snap["g_bias"]
        cur["W_user"][B:] = snap["W_user"][B:]
        cur["u_bias"][B:] = snap["u_bias"][B:]
        for name in SHARED:
            o.set_view(name, cur[name])
        o.update_csr(label, ng, nu, ni, idx, val)
        new = _views(o)
        for name, ids in (("g_bias", gids), ("W_item", iids), ("i_bias", iids), ("W_user", shared), ("u_bias", shared if user_bias else [])):
            for j in ids:
                c = (new[name][j] - snap[name][j]).astype(np.float32)
                acc[name][j] = (acc[name][j] + c).astype(np.float32)
                touched[name].add(j)
        cur = new
    out = cur
    for name in SHARED:
        lo = B if name in ("W_user", "u_bias") else 0
        out[name][lo:] = snap[name][lo:]
        for j in touched[name]:
            out[name][j] = (snap[name][j] + acc[name][j]).astype(np.float32)
        o.set_view(name, out[name])


def window_cuts(n, W):
    """the window sequence's cuts (svdf_wunit.cpp: wseq_from_csr): window w = rows [n w / W, n (w + 1) / W)"""
    return [(n * w // W, n * (w + 1) // W) for w in range(W)]


def simulate(o, d, B, W, passes, user_bias=True):
    for _ in range(passes):
        for b0, b1 in window_cuts(d.num_row, W):
            window_step(o, d.slice_rows(b0, b1), B, user_bias)
    return o


def shared_rows(rng, n, num_private, num_shared, num_item, num_global=0, max_g=0, max_shared=3, uvals=False, hot=(), hot_p=0.0,
                positions=("first", "middle", "last")):
    """rows of (globals, [private user + 1 .. max_shared shared ids], items); shared ids are num_private + j.  `hot` lists shared ids drawn
    with probability hot_p per row (many slots per window); the rest are drawn uniformly (rare: single-contribution applies).  The private entry
    sits first, in the middle or last of the user section, by `positions`."""
    rows = []
    for _ in range(n):
        g = sorted(int(x) for x in rng.choice(num_global, size=int(rng.integers(0, max_g + 1)), replace=False)) if num_global and max_g else []
        ns = int(rng.integers(0, max_shared + 1))
        sh = []
        if ns and hot and rng.random() < hot_p:
            sh.append(int(rng.choice(hot)))
        while len(sh) < ns:
            x = int(rng.integers(0, num_shared))
            if num_private + x not in sh:
                sh.append(num_private + x)
        sh = [(s, float(rng.choice([1.0, 0.5, 0.25, 2.0])) if uvals else 1.0) for s in sh]
        priv = (int(rng.integers(0, num_private)), float(rng.choice([1.0, 0.5, 1.5])) if uvals else 1.0)
        pos = str(rng.choice(list(positions)))
        at = 0 if pos == "first" else len(sh) if pos == "last" else (len(sh) + 1) // 2
        users = sh[:at] + [priv] + sh[at:]
        items = [(int(rng.integers(0, num_item)), 1.0)]
        rows.append((float(rng.integers(1, 6)), [(x, float(rng.uniform(0.1, 1.0))) for x in g], users, items))
    return CSRData.from_rows(rows)

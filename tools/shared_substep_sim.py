#!/usr/bin/env python3
"""CPU model (float64 numpy, no GPU) of the window step with hot shared user rows, beside tools/substep_sim.py (hot items): what ordered
sub-steps (knob window_shared_sub) do to the held-out RMSE at a given window size.  A toy, not the engine: users, items,
`buckets` shared user rows (bucket = user % buckets), pred = base + (p_u + s_b) . q_i, L2 decay, random labels 1 .. 5 as in
tools/sidefeat_window.py.

  sequential   every row against the current rows (the reference)
  stale        windows of --window rows: item rows and bucket rows are read as of the window start, their changes summed; private users exact
  sub-steps    the same, but a bucket row's slots are applied in file order --sub at a time, every sub-step against the row as the previous
               one left it (the private user's row as the walk held it at that data row)

Prints held-out RMSE minus the sequential pass's.
usage: python tools/shared_substep_sim.py --rows 200000 --window 2048 --sub 12"""
import argparse

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--users", type=int, default=20000)
ap.add_argument("--items", type=int, default=2000)
ap.add_argument("--buckets", type=int, default=64)
ap.add_argument("--factor", type=int, default=16)
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--window", type=int, default=2048)
ap.add_argument("--sub", type=int, default=12)
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()
LR, WD, BASE = 0.005, 0.004, 3.0
rng = np.random.default_rng(a.seed)
u, i = rng.integers(0, a.users, a.rows), rng.integers(0, a.items, a.rows)
y = rng.integers(1, 6, a.rows).astype(np.float64)
tu, ti = rng.integers(0, a.users, a.rows // 10), rng.integers(0, a.items, a.rows // 10)
ty = rng.integers(1, 6, a.rows // 10).astype(np.float64)
b = u % a.buckets


def init():
    r = np.random.default_rng(10)
    return [r.normal(0, 0.01, (n, a.factor)) for n in (a.users, a.buckets, a.items)]


def rmse(P, S, Q):
    pred = BASE + (((P[tu] + S[tu % a.buckets]) * Q[ti]).sum(1))
    return float(np.sqrt(np.mean((pred - ty) ** 2)))


def step(p, s, q, label):
    """new (p, s, q) of one row (update_no_decay + L2 decay)"""
    e = LR * (label - (BASE + (p + s) @ q))
    return (p + e * q) * (1 - LR * WD), (s + e * q) * (1 - LR * WD), (q + e * (p + s)) * (1 - LR * WD)


def run(window, sub):
    P, S, Q = init()
    for _ in range(a.passes):
        for w0 in range(0, a.rows, window):
            S0, Q0 = S.copy(), Q.copy()
            dS, dQ = np.zeros_like(S), np.zeros_like(Q)
            slots = [[] for _ in range(a.buckets)]
            for r in range(w0, min(w0 + window, a.rows)):
                ur, br, ir = u[r], b[r], i[r]
                if sub:
                    slots[br].append((r, P[ur].copy()))
                P[ur], s2, q2 = step(P[ur], S0[br], Q0[ir], y[r])
                dS[br] += s2 - S0[br]
                dQ[ir] += q2 - Q0[ir]
            Q = Q0 + dQ
            if not sub:
                S = S0 + dS
                continue
            for br in range(a.buckets):
                for j0 in range(0, len(slots[br]), sub):
                    acc = np.zeros(a.factor)
                    for r, p in slots[br][j0:j0 + sub]:
                        acc += step(p, S[br], Q0[i[r]], y[r])[1] - S[br]
                    S[br] = S[br] + acc
    return rmse(P, S, Q)


seq = run(1, 0)
print("sequential RMSE %.6f" % seq)
print("window %d, bucket rows stale: %+.2e" % (a.window, run(a.window, 0) - seq))
print("window %d, sub-steps of %d:   %+.2e" % (a.window, a.sub, run(a.window, a.sub) - seq))

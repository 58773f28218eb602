"""Checker of the ordered sub-steps for hot shared user rows in the window step (knob `window_shared_sub`; svdf_wunit.cpp, svdf_k_wunit.hip:
k_wunit_apply_shared), built on tests/side_table_sim.py (and through it tests/shared_user_sim.py) and the pinned C port of
the reference, one window at a time.

A shared user row (id >= B: a plain shared entry or a feature_user child) with MORE than `sub` slots in the window is hot there.  Everything
but the hot rows moves exactly as in side_table_sim.window_step -- every data row is the port's update_csr on the window-start shared rows, hot
ones included, and the private users walk on.  A hot row s is then applied in file order, `sub` slots at a time.  A slot is one data row r that
reaches s; its change is the port's update_csr on r with

  * every item row, item bias, global bias and every OTHER shared user row as of the window start,
  * r's private user row and bias as the walk held them when it reached r (before r's own update),
  * s and u_bias[s] as the previous sub-step left them,

and then new s - current s (row) and new u_bias[s] - current u_bias[s] (bias).  The changes of a sub-step are summed in slot order in fp32
(acc = +0 + c_1 + c_2 ...) and the row moves by the sum.

`hot_over` (default: sub) is the slot count above which a row is hot; hot_over = 0 with a sub-step as large as the window sends every shared
row through the lane in ONE sub-step, which must be side_table_sim.window_step bit for bit (tests/test_shared_hot_checker.py)."""
import numpy as np

import side_table_sim as sts
from shared_user_sim import SHARED, make_oracle, window_cuts   # noqa: F401


def _views(o):
    return {name: o.view(name).copy() for name in SHARED}


def window_step(o, d, B, sub, fu=(), fi=(), user_bias=True, hot_over=None):
    hot_over = sub if hot_over is None else hot_over
    rows, count = [], {}
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        users, items = sts.row_targets(idx, ng, nu, B, fu, fi)
        priv = [int(x) for x in idx[ng:ng + nu] if int(x) < B]
        rows.append((label, ng, nu, ni, idx, val, users, items, priv[0]))
        for u in users:
            count[u] = count.get(u, 0) + 1
    hot = {u for u, c in count.items() if c > hot_over} if sub > 0 else set()
    if not hot:
        return sts.window_step(o, d, B, fu, fi, user_bias)
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in SHARED}
    slots = {s: [] for s in hot}   # per hot row, in file order: (data row, its private user's row and bias before the data row's update)
    cur = {name: v.copy() for name, v in snap.items()}
    for r, (label, ng, nu, ni, idx, val, users, items, priv) in enumerate(rows):
        gids = [int(x) for x in idx[:ng]]
        cur["W_item"][...] = snap["W_item"]
        cur["i_bias"][...] = snap["i_bias"]
        cur["g_bias"][...] = snap["g_bias"]
        cur["W_user"][B:] = snap["W_user"][B:]
        cur["u_bias"][B:] = snap["u_bias"][B:]
        for s in users:
            if s in hot:
                slots[s].append((r, cur["W_user"][priv].copy(), np.float32(cur["u_bias"][priv])))
        for name in SHARED:
            o.set_view(name, cur[name])
        o.update_csr(label, ng, nu, ni, idx, val)
        new = _views(o)
        cold = [u for u in users if u not in hot]
        for name, ids in (("g_bias", gids), ("W_item", items), ("i_bias", items), ("W_user", cold), ("u_bias", cold if user_bias else [])):
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
    # ---- the hot rows, one after the other (each sees the others as of the window start)
    for s in sorted(hot):
        w, b = snap["W_user"][s].copy(), np.float32(snap["u_bias"][s])
        for s0 in range(0, len(slots[s]), sub):
            accw, accb = np.zeros_like(w), np.float32(0.0)
            for r, pw, pb in slots[s][s0:s0 + sub]:
                label, ng, nu, ni, idx, val, _, _, priv = rows[r]
                st = {name: snap[name].copy() for name in SHARED}
                st["W_user"][priv] = pw
                st["u_bias"][priv] = pb
                st["W_user"][s] = w
                st["u_bias"][s] = b
                for name in SHARED:
                    o.set_view(name, st[name])
                o.update_csr(label, ng, nu, ni, idx, val)
                accw = (accw + (o.view("W_user")[s] - w).astype(np.float32)).astype(np.float32)
                if user_bias:
                    accb = np.float32(accb + np.float32(np.float32(o.view("u_bias")[s]) - b))
            w = (w + accw).astype(np.float32)
            if user_bias:
                b = np.float32(b + accb)
        out["W_user"][s] = w
        out["u_bias"][s] = b
    for name in SHARED:
        o.set_view(name, out[name])


def simulate(o, d, B, W, passes, sub, fu=(), fi=(), user_bias=True, hot_over=None):
    for _ in range(passes):
        for b0, b1 in window_cuts(d.num_row, W):
            window_step(o, d.slice_rows(b0, b1), B, sub, fu, fi, user_bias, hot_over)
    return o

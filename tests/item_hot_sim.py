"""Checker of the ordered sub-steps for hot ITEM rows in the window step (knob `window_item_sub`; svdf_wunit.cpp, svdf_k_wunit.hip:
k_wunit_apply_hot<ITEM>), built on tests/side_table_sim.py / tests/shared_hot_sim.py and the pinned C port of the
reference, one window at a time.  It composes with the hot shared user rows of section 6k (knob `window_shared_sub`).

An item-range row -- a plain item entry's row, a feature_item child's row, or a row that is both -- with MORE than `isub` slots in the window
is hot there; a shared user row (id >= B) with more than `sub` slots is hot as in shared_hot_sim.  Everything but the hot rows moves exactly as
in side_table_sim.window_step -- every data row is the port's update_csr on the window-start shared rows, hot ones included, and the private
users walk on.  A hot row h is then applied in file order, its sub-step size at a time.  A slot is one data row r that reaches h; its change is
the port's update_csr on r with

  * every global bias, every shared user row and bias and every OTHER item row and item bias as of the window start (other hot rows too),
  * r's private user row and bias as the walk held them when it reached r (before r's own update),
  * h and its bias as the previous sub-step left them,

and then new h - current h (row) and new bias - current bias.  The changes of a sub-step are summed in slot order in fp32
(acc = +0 + c_1 + c_2 ...) and the row moves by the sum.  The item bias is always updated (as in the walk); a shared user row's bias only
with user_bias.

`ihot_over` / `hot_over` (default: the sub-step sizes) are the slot counts above which a row is hot; ihot_over = 0 with a sub-step as large as the
window sends every item row through the lane in ONE sub-step, which must be side_table_sim.window_step bit for bit
(tests/test_item_hot_checker.py)."""
import numpy as np

import shared_hot_sim as shs
import side_table_sim as sts
from shared_user_sim import SHARED, make_oracle, window_cuts   # noqa: F401


def _views(o):
    return {name: o.view(name).copy() for name in SHARED}


def item_slot_counts(d, B, fu=(), fi=()):
    """slots per item-range row in the window d (entries and feature_item children alike)"""
    c = {}
    for r in range(d.num_row):
        _, ng, nu, _, idx, _ = d.row(r)
        for i in sts.row_targets(idx, ng, nu, B, fu, fi)[1]:
            c[i] = c.get(i, 0) + 1
    return c


def window_step(o, d, B, isub, sub=0, fu=(), fi=(), user_bias=True, ihot_over=None, hot_over=None):
    ihot_over = isub if ihot_over is None else ihot_over
    hot_over = sub if hot_over is None else hot_over
    rows, ucount, icount = [], {}, {}
    for r in range(d.num_row):
        label, ng, nu, ni, idx, val = d.row(r)
        users, items = sts.row_targets(idx, ng, nu, B, fu, fi)
        priv = [int(x) for x in idx[ng:ng + nu] if int(x) < B]
        rows.append((label, ng, nu, ni, idx, val, users, items, priv[0]))
        for u in users:
            ucount[u] = ucount.get(u, 0) + 1
        for i in items:
            icount[i] = icount.get(i, 0) + 1
    ihot = {i for i, c in icount.items() if c > ihot_over} if isub > 0 else set()
    uhot = {u for u, c in ucount.items() if c > hot_over} if sub > 0 else set()
    if not ihot:
        return shs.window_step(o, d, B, sub, fu, fi, user_bias, hot_over)
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in SHARED}
    # per hot row, in file order: (data row, its private user's row and bias before the data row's update)
    uslots, islots = {s: [] for s in uhot}, {i: [] for i in ihot}
    cur = {name: v.copy() for name, v in snap.items()}
    for r, (label, ng, nu, ni, idx, val, users, items, priv) in enumerate(rows):
        gids = [int(x) for x in idx[:ng]]
        cur["W_item"][...] = snap["W_item"]
        cur["i_bias"][...] = snap["i_bias"]
        cur["g_bias"][...] = snap["g_bias"]
        cur["W_user"][B:] = snap["W_user"][B:]
        cur["u_bias"][B:] = snap["u_bias"][B:]
        for s in users:
            if s in uhot:
                uslots[s].append((r, cur["W_user"][priv].copy(), np.float32(cur["u_bias"][priv])))
        for i in items:
            if i in ihot:
                islots[i].append((r, cur["W_user"][priv].copy(), np.float32(cur["u_bias"][priv])))
        for name in SHARED:
            o.set_view(name, cur[name])
        o.update_csr(label, ng, nu, ni, idx, val)
        new = _views(o)
        ucold = [u for u in users if u not in uhot]
        icold = [i for i in items if i not in ihot]
        for name, ids in (("g_bias", gids), ("W_item", icold), ("i_bias", icold), ("W_user", ucold), ("u_bias", ucold if user_bias else [])):
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
    # ---- the hot rows, one after the other (each sees all the others, user or item, as of the window start)
    lanes = [("W_user", "u_bias", s, uslots[s], sub, user_bias) for s in sorted(uhot)] + \
            [("W_item", "i_bias", i, islots[i], isub, True) for i in sorted(ihot)]
    for wname, bname, h, slots, step, with_bias in lanes:
        w, b = snap[wname][h].copy(), np.float32(snap[bname][h])
        for s0 in range(0, len(slots), step):
            accw, accb = np.zeros_like(w), np.float32(0.0)
            for r, pw, pb in slots[s0:s0 + step]:
                label, ng, nu, ni, idx, val, _, _, priv = rows[r]
                st = {name: snap[name].copy() for name in SHARED}
                st["W_user"][priv] = pw
                st["u_bias"][priv] = pb
                st[wname][h] = w
                st[bname][h] = b
                for name in SHARED:
                    o.set_view(name, st[name])
                o.update_csr(label, ng, nu, ni, idx, val)
                accw = (accw + (o.view(wname)[h] - w).astype(np.float32)).astype(np.float32)
                if with_bias:
                    accb = np.float32(accb + np.float32(np.float32(o.view(bname)[h]) - b))
            w = (w + accw).astype(np.float32)
            if with_bias:
                b = np.float32(b + accb)
        out[wname][h] = w
        out[bname][h] = b
    for name in SHARED:
        o.set_view(name, out[name])


def simulate(o, d, B, W, passes, isub, sub=0, fu=(), fi=(), user_bias=True, ihot_over=None, hot_over=None):
    for _ in range(passes):
        for b0, b1 in window_cuts(d.num_row, W):
            window_step(o, d.slice_rows(b0, b1), B, isub, sub, fu, fi, user_bias, ihot_over, hot_over)
    return o

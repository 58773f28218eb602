"""Checker of the ordered sub-steps for hot ITEM rows of user-group (SVD++) blocks in the window step (knob `window_block_item_sub`;
svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_walk<LPI, true, true> and k_wunit_apply_hot<LPI, true, true>), built on
tests/block_shared_sim.py and the pinned C port of the reference the way tests/block_hot_sim.py is, one window at a time.  It composes with
the hot shared user rows of section 6q (knob `window_block_sub`), as item_hot_sim composes sections 6m and 6k.

An item row with MORE than `isub` slots in the window is hot there; a shared user row (id >= B) with more than `sub` slots is hot as in
block_hot_sim.  Everything but the hot rows moves exactly as in block_shared_sim.window_step -- every data row is the port's
SVDPPFeature::update on the window-start shared rows, hot ones included, and the private users and their spans' tmp_ufeedback walk on; the
pass also notes every span's private row and bias at the span's start and, for the assertion below, before every row that holds a hot entry.
A hot row h is then applied in file order, its sub-step size at a time.  A slot is one data row r = row i of a span that reaches h; its
change is the port's update on r with

  * every OTHER item row and item bias, every global bias, feedback row and feedback bias and every shared user row as of the window start
    (other hot rows of either side too),
  * the span's private row and bias and its tmp_ufeedback / tmp_ufeedback_bias as the walk held them when it reached r.  The port's
    tmp_ufeedback is not a view, so the span is REPLAYED from its start: before every replayed row the shared state is set back to the
    snapshot, the private row is the noted start value before row 0 and is left as it evolves after that, and rows 0 .. i - 1 go in as
    START / MIDDLE blocks -- the main pass again, which the checker asserts on the private row and bias before row i;
  * h and its bias as the previous sub-step left them, set just before row i,

and then new h - current h (row) and new bias - current bias.  The rest of the span is fed so that the port's span closes, and discarded.
The changes of a sub-step are summed in slot order in fp32 (acc = +0 + c_1 + c_2 ...) and the row moves by the sum.  The item bias is always
updated (as in the walk); a shared user row's bias only with user_bias.  Hot rows are taken one after the other, each seeing the others as of
the window start: a data row with two hot entries gives one slot to each.

`ihot_over` / `hot_over` (default: the sub-step sizes) are the slot counts above which a row is hot; ihot_over = 0 with a sub-step as large
as the window sends every item row through the lane in ONE sub-step, which must be block_shared_sim.window_step bit for bit
(tests/test_block_item_hot_checker.py)."""
import numpy as np

import block_hot_sim as bhs
import block_shared_sim as bss
from block_hot_sim import _bias, _row_blocks, _row_ids, _tag
from block_shared_sim import VIEWS, make_oracle, shared_blocks, window_cuts   # noqa: F401
from svdfeature_amd.data import TAG_DEFAULT, TAG_END


def item_slot_counts(blocks):
    """how many slots (item entries of data rows) every item id meets in the window"""
    count = {}
    for _, _, d in bss.spans(blocks):
        for r in range(d.num_row):
            _, ng, nu, _, idx, _ = d.row(r)
            for i in idx[ng + nu:]:
                count[int(i)] = count.get(int(i), 0) + 1
    return count


def window_step(o, blocks, B, isub, sub=0, user_bias=True, ihot_over=None, hot_over=None):
    """one window on the user-group oracle trainer o (user ids >= B are shared rows; B = num_user: none); returns (hot user rows, hot item rows)"""
    ihot_over = isub if ihot_over is None else ihot_over
    hot_over = sub if hot_over is None else hot_over
    ihot = {i for i, c in item_slot_counts(blocks).items() if c > ihot_over} if isub > 0 else set()
    if not ihot:
        return bhs.window_step(o, blocks, B, sub, user_bias, hot_over), 0
    uhot = {s for s, c in bhs.slot_counts(blocks, B).items() if c > hot_over} if sub > 0 else set()
    sp = bss.spans(blocks)
    fed = [_row_blocks(*x) for x in sp]
    snap = bss._views(o)
    has_b = snap["u_bias"].size > 0
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in VIEWS}
    cur = {name: v.copy() for name, v in snap.items()}
    uslots, islots = {s: [] for s in uhot}, {i: [] for i in ihot}   # per hot row, in file order: (span, row of the span)
    start, before = [], {}   # the span's private row and bias at its start; before every row that holds a hot entry (the assertion)

    def reset_shared(st):
        for name in VIEWS:
            lo = B if name in ("W_user", "u_bias") else 0
            st[name][lo:] = snap[name][lo:]

    # ---- block_shared_sim.window_step, the hot rows left out of the sums
    for q, (fbi, fbv, d) in enumerate(sp):
        n = d.num_row
        for r in range(n):
            tag = _tag(n, r)
            gids, shared, priv, iids = _row_ids(d, r, B)
            if r == 0:
                start.append((priv, cur["W_user"][priv].copy(), _bias(cur, priv)))
            for s in shared:
                if s in uhot:
                    uslots[s].append((q, r))
            for i in iids:
                if i in ihot:
                    islots[i].append((q, r))
            if any(s in uhot for s in shared) or any(i in ihot for i in iids):
                before[(q, r)] = (cur["W_user"][priv].copy(), _bias(cur, priv))
            fids = [int(x) for x in fbi] if tag in (TAG_DEFAULT, TAG_END) else []
            reset_shared(cur)
            bss._set(o, cur)
            o.update_block(fed[q][r])
            new = bss._views(o)
            ucold = [s for s in shared if s not in uhot]
            icold = [i for i in iids if i not in ihot]
            for name, ids in (("g_bias", gids), ("W_item", icold), ("i_bias", icold), ("W_user", ucold), ("u_bias", ucold if user_bias else []),
                              ("W_ufeedback", fids), ("ufeedback_bias", fids if user_bias else [])):
                for j in ids:
                    c = (new[name][j] - snap[name][j]).astype(np.float32)
                    acc[name][j] = (acc[name][j] + c).astype(np.float32)
                    touched[name].add(j)
            cur = new
    out = cur
    reset_shared(out)
    for name in VIEWS:
        for j in touched[name]:
            out[name][j] = (snap[name][j] + acc[name][j]).astype(np.float32)
    # ---- the hot rows, one after the other (each sees all the others, user or item, as of the window start)
    lanes = [("W_user", "u_bias", s, uslots[s], sub, user_bias, has_b) for s in sorted(uhot)] + \
            [("W_item", "i_bias", i, islots[i], isub, True, True) for i in sorted(ihot)]
    for wname, bname, h, slots, step, with_bias, set_b in lanes:
        w = snap[wname][h].copy()
        b = np.float32(snap[bname][h]) if set_b else np.float32(0.0)
        for s0 in range(0, len(slots), step):
            accw, accb = np.zeros_like(w), np.float32(0.0)
            for q, i in slots[s0:s0 + step]:
                fbi, fbv, d = sp[q]
                priv, pw, pb = start[q]
                st = {name: v.copy() for name, v in snap.items()}
                st["W_user"][priv] = pw
                if has_b:
                    st["u_bias"][priv] = pb
                for r in range(d.num_row):   # the span from its start; the rows after i only close the port's span
                    reset_shared(st)
                    if r == i:
                        bw, bb = before[(q, i)]
                        assert np.array_equal(st["W_user"][priv].view(np.uint32), bw.view(np.uint32)), "the replay left the walk's private row"
                        assert _bias(st, priv).view(np.uint32) == bb.view(np.uint32), "the replay left the walk's private bias"
                        st[wname][h] = w
                        if set_b:
                            st[bname][h] = b
                    bss._set(o, st)
                    o.update_block(fed[q][r])
                    nu, nb = o.view("W_user"), (o.view("u_bias") if has_b else None)
                    if r == i:
                        accw = (accw + (o.view(wname)[h] - w).astype(np.float32)).astype(np.float32)
                        if with_bias:
                            accb = np.float32(accb + np.float32(np.float32(o.view(bname)[h]) - b))
                    st["W_user"][priv] = nu[priv]
                    if has_b:
                        st["u_bias"][priv] = nb[priv]
            w = (w + accw).astype(np.float32)
            if with_bias:
                b = np.float32(b + accb)
        out[wname][h] = w
        if set_b:
            out[bname][h] = b
    bss._set(o, out)
    return len(uhot), len(ihot)


def simulate(o, ba, B, W, passes, isub, sub=0, user_bias=True, ihot_over=None, hot_over=None, cuts=None):
    """`passes` passes over the block sequence in W windows (or the given cuts); returns the hot rows applied (user rows, item rows): the library's
    counters 35 and 36"""
    blocks = ba.to_blocks()
    nu, ni = 0, 0
    for _ in range(passes):
        for b0, b1 in (cuts or window_cuts(ba, W)):
            a, b = window_step(o, blocks[b0:b1], B, isub, sub, user_bias, ihot_over, hot_over)
            nu, ni = nu + a, ni + b
    return nu, ni

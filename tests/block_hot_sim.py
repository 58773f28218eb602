"""Checker of the ordered sub-steps for hot shared user rows of user-group (SVD++) blocks in the window step (knob `window_block_sub`;
svdf_wunit.cpp, svdf_k_wunit.hip: k_wunit_walk<LPI, true, true> and k_wunit_apply_hot<LPI, false, true>), built on
tests/block_shared_sim.py and the pinned C port of the reference, one window at a time.

A shared user row (id >= B) with MORE than `sub` slots in the window is hot there.  Everything but the hot rows moves exactly as in
block_shared_sim.window_step -- every data row is the port's SVDPPFeature::update on the window-start shared rows, hot ones included, and the
private users and their spans' tmp_ufeedback walk on; the pass also notes every span's private row and bias at the span's start and, for the
assertion below, before every row.  A hot row s is then applied in file order, `sub` slots at a time.  A slot is one data row r = row i of a
span that reaches s; its change is the port's update on r with

  * every item row, item bias, global bias, feedback row and feedback bias and every OTHER shared user row as of the window start,
  * the span's private row and bias and its tmp_ufeedback / tmp_ufeedback_bias as the walk held them when it reached r.  The port's
    tmp_ufeedback is not a view, so the span is REPLAYED from its start: before every replayed row the shared state is set back to the snapshot,
    the private row is the noted start value before row 0 and is left as it evolves after that, and rows 0 .. i - 1 go in as START / MIDDLE
    blocks -- the main pass again, which the checker asserts on the private row and bias before row i;
  * s and u_bias[s] as the previous sub-step left them, set just before row i,

and then new s - current s (row) and new u_bias[s] - current u_bias[s] (bias).  The rest of the span is fed so that the port's span closes,
and discarded.  The changes of a sub-step are summed in slot order in fp32 (acc = +0 + c_1 + c_2 ...) and the row moves by the sum.  Hot rows
are taken one after the other, each seeing the others as of the window start.

`hot_over` (default: sub) is the slot count above which a row is hot; hot_over = 0 with a sub-step as large as the window sends every shared
row through the lane in ONE sub-step, which must be block_shared_sim.window_step bit for bit (tests/test_block_hot_checker.py)."""
import numpy as np

import block_shared_sim as bss
from block_shared_sim import VIEWS, make_oracle, shared_blocks, window_cuts   # noqa: F401
from svdfeature_amd import PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

EMPTY = np.zeros(0, np.uint32), np.zeros(0, np.float32)


def _tag(n, r):
    return TAG_DEFAULT if n == 1 else TAG_START if r == 0 else TAG_END if r == n - 1 else TAG_MIDDLE


def _row_blocks(fbi, fbv, d):
    """the span's rows as the blocks they are fed as: one row DEFAULT; more: START, MIDDLE ..., END"""
    n = d.num_row
    return [PlusBlock(*((fbi, fbv) if _tag(n, r) != TAG_MIDDLE else EMPTY), d.slice_rows(r, r + 1), _tag(n, r)) for r in range(n)]


def _bias(st, j):
    return np.float32(st["u_bias"][j]) if st["u_bias"].size else np.float32(0.0)   # (no view without user biases)


def _row_ids(d, r, B):
    _, ng, nu, ni, idx, _ = d.row(r)
    users = [int(x) for x in idx[ng:ng + nu]]
    return [int(x) for x in idx[:ng]], [u for u in users if u >= B], [u for u in users if u < B][0], [int(x) for x in idx[ng + nu:]]


def slot_counts(blocks, B):
    """how many slots (data rows) every shared user id meets in the window"""
    count = {}
    for _, _, d in bss.spans(blocks):
        for r in range(d.num_row):
            for s in _row_ids(d, r, B)[1]:
                count[s] = count.get(s, 0) + 1
    return count


def window_step(o, blocks, B, sub, user_bias=True, hot_over=None):
    """one window on the user-group oracle trainer o; returns the number of hot rows"""
    hot_over = sub if hot_over is None else hot_over
    hot = {s for s, c in slot_counts(blocks, B).items() if c > hot_over} if sub > 0 else set()
    if not hot:
        bss.window_step(o, blocks, B, user_bias)
        return 0
    sp = bss.spans(blocks)
    fed = [_row_blocks(*x) for x in sp]
    snap = bss._views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in VIEWS}
    cur = {name: v.copy() for name, v in snap.items()}
    slots = {s: [] for s in hot}   # per hot row, in file order: (span, row of the span)
    start, before = [], {}         # the span's private row and bias at its start; before every row that holds a hot entry (the assertion)

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
                if s in hot:
                    slots[s].append((q, r))
                    before[(q, r)] = (cur["W_user"][priv].copy(), _bias(cur, priv))
            fids = [int(x) for x in fbi] if tag in (TAG_DEFAULT, TAG_END) else []
            reset_shared(cur)
            bss._set(o, cur)
            o.update_block(fed[q][r])
            new = bss._views(o)
            cold = [s for s in shared if s not in hot]
            for name, ids in (("g_bias", gids), ("W_item", iids), ("i_bias", iids), ("W_user", cold), ("u_bias", cold if user_bias else []),
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
    # ---- the hot rows, one after the other (each sees the others as of the window start)
    for s in sorted(hot):
        w, b = snap["W_user"][s].copy(), _bias(snap, s)
        has_b = snap["u_bias"].size > 0
        for s0 in range(0, len(slots[s]), sub):
            accw, accb = np.zeros_like(w), np.float32(0.0)
            for q, i in slots[s][s0:s0 + sub]:
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
                        st["W_user"][s] = w
                        if has_b:
                            st["u_bias"][s] = b
                    bss._set(o, st)
                    o.update_block(fed[q][r])
                    nu, nb = o.view("W_user"), (o.view("u_bias") if has_b else None)
                    if r == i:
                        accw = (accw + (nu[s] - w).astype(np.float32)).astype(np.float32)
                        if user_bias:
                            accb = np.float32(accb + np.float32(np.float32(nb[s]) - b))
                    st["W_user"][priv] = nu[priv]
                    if has_b:
                        st["u_bias"][priv] = nb[priv]
            w = (w + accw).astype(np.float32)
            if user_bias:
                b = np.float32(b + accb)
        out["W_user"][s] = w
        if has_b:
            out["u_bias"][s] = b
    bss._set(o, out)
    return len(hot)


def simulate(o, ba, B, W, passes, sub, user_bias=True, hot_over=None, cuts=None):
    """`passes` passes over the block sequence in W windows (or the given cuts); returns the hot rows applied, the library's counter 35"""
    blocks = ba.to_blocks()
    nhot = 0
    for _ in range(passes):
        for b0, b1 in (cuts or window_cuts(ba, W)):
            nhot += window_step(o, blocks[b0:b1], B, sub, user_bias, hot_over)
    return nhot

"""Checker of the window step for user-group (SVD++) blocks whose rows carry shared user ids (`amd:shared_user_from = B` on a format_type 1
trainer; svdf_wunit.cpp, svdf_k_wunit.hip, svdf_k_wave.hip), built on the pinned C port of the reference
(oracle.OracleTrainer("port", 1, ...)), one window at a time:

  * snapshot of the shared state: W_item, i_bias, g_bias, the rows >= B of W_user / u_bias, W_ufeedback and ufeedback_bias;
  * a DEFAULT block or a START..END span is the reference's SVDPPFeature::update fed ROW BY ROW -- one row: a DEFAULT block; more: the first as a
    START block, the last as an END block, the others as MIDDLE blocks, so that prepare_ufeedback runs before the first row and update_ufeedback
    after the last; before every row the shared state is set back to the snapshot (the private user row and bias and the port's tmp_ufeedback
    keep what the walk holds), and new - snapshot of every target the row touches is added, in fp32 and in file order, to the target's
    accumulator (acc = +0 + c_1 + c_2 ...); W_ufeedback's change is taken at the END;
  * at the window's end every touched target becomes snapshot + acc.

Blocks with one user entry per row make this oracle.update_block_stale plus the window's add; blocks with empty feedback lists make it
shared_user_sim.window_step on the same rows: tests/test_block_shared_checker.py pins both bit for bit."""
import numpy as np

from oracle import oracle
from svdfeature_amd import BlockArrays, CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias")


def make_oracle(conf, seed=10, active=0):
    t = oracle.OracleTrainer("port", 1, active)
    t.seed(seed)
    for k, v in conf:
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    return t


def _views(o):
    out = {}
    for name in VIEWS:
        v = o.view(name)
        out[name] = np.zeros(0, np.float32) if v is None else v.copy()
    return out


def _set(o, views):
    for name, v in views.items():
        if v.size:
            o.set_view(name, v)


def spans(blocks):
    """the DEFAULT blocks and START..END spans of a block list: (feedback ids, feedback values, CSRData of the span's rows in file order)"""
    out, rows, fb = [], None, None
    for b in blocks:
        if b.extend_tag in (TAG_DEFAULT, TAG_START):
            assert rows is None, "a START block inside an open span"
            rows, fb = [], (b.index_ufeedback, b.value_ufeedback)
        else:
            assert rows is not None, "MIDDLE / END block without a START"
        rows.append(b.data)
        if b.extend_tag in (TAG_DEFAULT, TAG_END):
            out.append((fb[0], fb[1], CSRData.concat(rows)))
            rows = None
    assert rows is None, "the window ends inside a START..END span"
    return out


def window_step(o, blocks, B, user_bias=True):
    """one window (PlusBlocks in file order, every span closed) on the user-group oracle trainer o; user ids >= B are shared rows"""
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in VIEWS}
    cur = {name: v.copy() for name, v in snap.items()}
    empty = np.zeros(0, np.uint32), np.zeros(0, np.float32)
    for fbi, fbv, d in spans(blocks):
        n = d.num_row
        for r in range(n):
            tag = TAG_DEFAULT if n == 1 else TAG_START if r == 0 else TAG_END if r == n - 1 else TAG_MIDDLE
            _, ng, nu, ni, idx, _ = d.row(r)
            gids = [int(x) for x in idx[:ng]]
            shared = [int(x) for x in idx[ng:ng + nu] if x >= B]
            iids = [int(x) for x in idx[ng + nu:]]
            fids = [int(x) for x in fbi] if tag in (TAG_DEFAULT, TAG_END) else []
            # the shared parts as they were at the window start; the private user rows as they are now
            for name in VIEWS:
                lo = B if name in ("W_user", "u_bias") else 0
                cur[name][lo:] = snap[name][lo:]
            _set(o, cur)
            f = (fbi, fbv) if tag != TAG_MIDDLE else empty
            o.update_block(PlusBlock(f[0], f[1], d.slice_rows(r, r + 1), tag))
            new = _views(o)
            for name, ids in (("g_bias", gids), ("W_item", iids), ("i_bias", iids), ("W_user", shared), ("u_bias", shared if user_bias else []),
                              ("W_ufeedback", fids), ("ufeedback_bias", fids if user_bias else [])):
                for j in ids:
                    c = (new[name][j] - snap[name][j]).astype(np.float32)
                    acc[name][j] = (acc[name][j] + c).astype(np.float32)
                    touched[name].add(j)
            cur = new
    for name in VIEWS:
        lo = B if name in ("W_user", "u_bias") else 0
        cur[name][lo:] = snap[name][lo:]
        for j in touched[name]:
            cur[name][j] = (snap[name][j] + acc[name][j]).astype(np.float32)
    _set(o, cur)


def window_cuts(ba, W):
    """the block sequence's cuts (svdf_wunit.cpp: wseq_from_blocks): even block positions moved forward to where no span is open"""
    nb, tag = ba.num_block, ba.extend_tag
    cut = [0]
    for w in range(1, W):
        pos = max(nb * w // W, cut[-1])
        while 0 < pos < nb and tag[pos - 1] in (TAG_START, TAG_MIDDLE):
            pos += 1
        cut.append(pos)
    cut.append(nb)
    return list(zip(cut[:-1], cut[1:]))


def simulate(o, ba, B, W, passes, user_bias=True):
    blocks = ba.to_blocks()
    for _ in range(passes):
        for b0, b1 in window_cuts(ba, W):
            window_step(o, blocks[b0:b1], B, user_bias)
    return o


def shared_blocks(rng, nblocks, num_private, num_shared, num_item, num_fb, max_rows=7, max_fb=5, max_shared=3, uvals=False, per_row=False,
                  positions=("first", "middle", "last"), split_every=4, num_global=0, binary=False, min_shared=0, fb_sizes=None, long_unit=0,
                  single=False):
    """user-group blocks of (private user + min_shared .. max_shared shared ids, one item): the shared ids (num_private + j) are attributes of
    the USER -- the same section on every row of a block -- unless per_row, where every row draws its own.  Every split_every'th block of 3+
    rows is a START / MIDDLE / END span.  uvals: non-unit values on the shared entries (private values stay 1 unless uvals == "all").
    fb_sizes: the feedback lists' lengths, in turn; long_unit: block 2 has that many rows; single: the LAST block is one row whose shared id
    (the last one, which nobody else draws) meets no other row -- its change is applied in place."""
    blocks = []
    draw_shared = num_shared - 1 if single else num_shared
    for b in range(nblocks):
        uid = int(rng.integers(0, num_private))
        last_single = single and b == nblocks - 1
        nrow = 1 if last_single else long_unit if long_unit and b == 2 else int(rng.integers(1, max_rows + 1))
        nfb = int(fb_sizes[b % len(fb_sizes)]) if fb_sizes else 0 if b % 7 == 3 or max_fb == 0 else int(rng.integers(1, max_fb + 1))
        fbi = np.sort(rng.choice(num_fb, size=nfb, replace=False)).astype(np.uint32)
        fbv = np.full(nfb, 1.0 / np.sqrt(max(nfb, 1)), np.float32)

        def section():
            ns = int(rng.integers(min_shared, max_shared + 1))
            sh = [num_private + int(x) for x in rng.choice(draw_shared, size=ns, replace=False)]
            if last_single:
                sh = sh[:1] + [num_private + num_shared - 1]
            sh = [(s, float(rng.choice([1.0, 0.5, 0.25, 2.0])) if uvals else 1.0) for s in sh]
            pos = str(rng.choice(list(positions)))
            at = 0 if pos == "first" else len(sh) if pos == "last" else (len(sh) + 1) // 2
            pv = float(rng.choice([1.0, 0.5, 1.5])) if uvals == "all" else 1.0
            return sh[:at] + [(uid, pv)] + sh[at:]

        sec = section()
        rows = []
        for _ in range(nrow):
            g = [(int(rng.integers(0, num_global)), float(rng.uniform(0.1, 1.0)))] if num_global else []
            label = float(rng.integers(0, 2)) if binary else float(rng.integers(1, 6))
            rows.append((label, g, section() if per_row else sec, [(int(rng.integers(0, num_item)), 1.0)]))
        d = CSRData.from_rows(rows)
        if split_every and b % split_every == 1 and nrow >= 3:
            e = np.zeros(0, np.uint32), np.zeros(0, np.float32)
            blocks.append(PlusBlock(fbi, fbv, d.slice_rows(0, 1), TAG_START))
            blocks.append(PlusBlock(e[0], e[1], d.slice_rows(1, nrow - 1), TAG_MIDDLE))
            blocks.append(PlusBlock(fbi, fbv, d.slice_rows(nrow - 1, nrow), TAG_END))
        else:
            blocks.append(PlusBlock(fbi, fbv, d, TAG_DEFAULT))
    return blocks

"""The CPU checker of the window step (`amd:step = minibatch`; svdf_wunit.cpp, svdf_k_wunit.hip, svdf_k_wave.hip; DESIGN.md sections 6i, 6j,
6k, 6m, 6p, 6q, 6u), built on the pinned C port of the reference (oracle.OracleTrainer("port")).  The reference has no minibatch step, so this
module states the rule, once, for data rows (step_rows: the port's update_csr) and for user-group SVD++ blocks (step_blocks: the port's
update_block); tests/test_shared_hot_checker.py, test_item_hot_checker.py and test_block_item_hot_checker.py pin it to the checkers outside this
family and to recorded results.

One window, on a trainer whose user ids >= B are SHARED rows (`amd:shared_user_from = B`) and whose ids < B are private (one per data row):

  * SNAPSHOT.  The shared state is W_item, i_bias, g_bias, the rows >= B of W_user / u_bias, and W_ufeedback / ufeedback_bias: as of the
    window start.
  * WALK.  The data rows go in file order.  Before every row the shared state is set back to the snapshot -- the private user row and bias
    (and, inside a block, the port's tmp_ufeedback) keep what the walk holds -- and the row is the port's update.  A block, or a
    START..MIDDLE..END span of blocks, is fed ROW BY ROW: one row as a DEFAULT block; more as START, MIDDLE ..., END, so that
    prepare_ufeedback runs before the first row and update_ufeedback after the last.  new - snapshot of every TARGET the row touches is
    added, in fp32 and in file order, to the target's accumulator (acc = +0 + c_1 + c_2 ...).  The targets are the row's global entries, its
    item entries and shared user entries, the children that the feature_item / feature_user tables (which the port has loaded too) give its
    item and user entries, and, at a span's last row, the span's feedback ids.  User-side biases only with user_bias.
  * WRITE.  At the window's end every touched target becomes snapshot + acc.
  * LANES (knobs window_shared_sub / window_item_sub, window_block_sub / window_block_item_sub).  A shared user row with MORE than `sub` slots
    in the window, or an item-range row (entry, child, or both) with more than `isub`, is HOT there; a slot is one data row that reaches it.
    `hot_over` / `ihot_over` replace the two thresholds (0 with a sub-step as large as the window: every row rides the lane in ONE sub-step,
    which is the walk's own sum).  The walk leaves hot rows out of its sums.  A hot row h is then applied in file order, its sub-step size
    at a time.  A slot's change is the port's update on its data row with

      - everything shared as of the window start, other hot rows of either side included,
      - the span's private row and bias and its tmp_ufeedback as the walk held them on reaching the data row.  tmp_ufeedback is not a view,
        so the span is REPLAYED from its start (a plain data row is a span of one): the private row as the walk held it at the span's start,
        the shared state set back before every row -- the walk again, which the checker asserts on the private row and bias,
      - h and its bias as the previous sub-step left them, set just before the data row,

    and then new h - current h (row) and new bias - current bias.  The rest of the span is fed so that the port's span closes, and discarded.
    The changes of a sub-step are summed in slot order in fp32 and the row moves by the sum.  The item bias always moves; a shared user
    row's only with user_bias.  Hot rows are taken one after the other: a data row with two hot entries gives one slot to each.

Without lanes a row's private entry is never looked for."""
import collections

import numpy as np

from oracle import oracle
from svdfeature_amd import CSRData, PlusBlock
from svdfeature_amd.data import TAG_DEFAULT, TAG_END, TAG_MIDDLE, TAG_START

VIEWS = ("W_user", "u_bias", "W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias")
SHARED = ("W_item", "i_bias", "g_bias", "W_user", "u_bias")   # the views of a trainer without feedback
EMPTY = np.zeros(0, np.uint32), np.zeros(0, np.float32)


def make_oracle(conf, seed=10, active=0, user_group=False):
    t = oracle.OracleTrainer("port", int(user_group), active)
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


# ---- side tables and targets

def read_table(path):
    """a feature_user / feature_item text table (apex-utils/apex_utils.h:172-195, ``n idx:val ...`` per id) -> per id a list of
    (child id, value)"""
    with open(path) as f:
        tok = f.read().split()
    rows, p = [], 0
    while p < len(tok):
        n = int(tok[p])
        rows.append([(int(t.split(":")[0]), float(np.float32(t.split(":")[1]))) for t in tok[p + 1:p + 1 + n]])
        p += 1 + n
    return rows


def write_table(path, rows):
    with open(path, "w") as f:
        for row in rows:
            f.write(("%d %s" % (len(row), " ".join("%d:%.9g" % (c, v) for c, v in row))).strip() + "\n")
    return path


def children(table, ids):
    out = []
    for x in ids:
        if x < len(table):
            out += [c for c, _ in table[x]]
    return out


def row_targets(idx, ng, nu, B, fu, fi):
    """(shared user rows, item rows) one row touches: its shared user entries and item entries, then the children the tables give"""
    uids = [int(x) for x in idx[ng:ng + nu]]
    iids = [int(x) for x in idx[ng + nu:]]
    return [u for u in uids if u >= B] + children(fu, uids), iids + children(fi, iids)


def reaches_twice(d, r, B, fu, fi):
    _, ng, nu, _, idx, _ = d.row(r)
    us, its = row_targets(idx, ng, nu, B, fu, fi)
    return len(set(us)) != len(us) or len(set(its)) != len(its)


def drop_rows_reaching_twice(d, B, fu, fi):
    """the window step refuses a row that touches one target twice after expansion: keep the others"""
    keep = np.array([not reaches_twice(d, r, B, fu, fi) for r in range(d.num_row)], bool)
    return d.select_rows(keep)


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


# one data row's targets: global ids, all its user ids, (shared user rows, item rows) as row_targets gives them, feedback ids
Row = collections.namedtuple("Row", "gids uids users items fids")


def _rows(d, B, fu=(), fi=(), fids=()):
    """the Rows of CSRData d; the feedback ids go to the last one"""
    out = []
    for r in range(d.num_row):
        _, ng, nu, _, idx, _ = d.row(r)
        users, items = row_targets(idx, ng, nu, B, fu, fi)
        out.append(Row([int(x) for x in idx[:ng]], [int(x) for x in idx[ng:ng + nu]], users, items, list(fids) if r == d.num_row - 1 else []))
    return out


def _counts(id_lists):
    count = {}
    for ids in id_lists:
        for j in ids:
            count[j] = count.get(j, 0) + 1
    return count


def item_slot_counts(d, B, fu=(), fi=()):
    """slots per item-range row in the window d (entries and feature_item children alike)"""
    return _counts(row.items for row in _rows(d, B, fu, fi))


def slot_counts(blocks, B):
    """how many slots (data rows) every shared user id meets in the window of blocks"""
    return _counts(row.users for _, _, d in spans(blocks) for row in _rows(d, B))


def block_item_slot_counts(blocks):
    """how many slots (item entries of data rows) every item id meets in the window of blocks"""
    return _counts(row.items for _, _, d in spans(blocks) for row in _rows(d, 0))


# ---- the window rule

def _window(o, B, spans_, feed, sub, isub, user_bias, hot_over, ihot_over):
    """one window on oracle trainer o: spans_ is a list of spans, each a list of Rows; feed(q, r) is the port's update on row r of span q.
    Returns (hot user rows, hot item rows)."""
    def hot(id_lists, step, over):
        over = step if over is None else over
        return {j for j, c in _counts(id_lists).items() if c > over} if step > 0 else set()

    every = [row for span in spans_ for row in span]
    uhot, ihot = hot((row.users for row in every), sub, hot_over), hot((row.items for row in every), isub, ihot_over)
    snap = _views(o)
    acc = {name: np.zeros_like(v) for name, v in snap.items()}
    touched = {name: set() for name in VIEWS}
    slots = {("W_user", s): [] for s in uhot}   # per hot row, in file order: (span, row of the span)
    slots.update({("W_item", i): [] for i in ihot})
    before = {}   # (span, row) -> the span's private user, its row and bias before the data row's update (lanes only)

    def reset_shared(st):
        for name in VIEWS:
            lo = B if name in ("W_user", "u_bias") else 0
            st[name][lo:] = snap[name][lo:]

    # ---- the walk, the hot rows left out of the sums
    cur = {name: v.copy() for name, v in snap.items()}
    for q, span in enumerate(spans_):
        for r, row in enumerate(span):
            if slots:
                priv = [u for u in row.uids if u < B][0]
                before[q, r] = priv, cur["W_user"][priv].copy(), np.float32(cur["u_bias"][priv])
            for key in [("W_user", s) for s in row.users] + [("W_item", i) for i in row.items]:
                if key in slots:
                    slots[key].append((q, r))
            reset_shared(cur)
            _set(o, cur)
            feed(q, r)
            new = _views(o)
            ucold = [s for s in row.users if s not in uhot]
            icold = [i for i in row.items if i not in ihot]
            for name, ids in (("g_bias", row.gids), ("W_item", icold), ("i_bias", icold), ("W_user", ucold), ("u_bias", ucold if user_bias else []),
                              ("W_ufeedback", row.fids), ("ufeedback_bias", row.fids if user_bias else [])):
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
    lanes = [("W_user", "u_bias", s, sub, user_bias) for s in sorted(uhot)] + [("W_item", "i_bias", i, isub, True) for i in sorted(ihot)]
    for wname, bname, h, step, with_bias in lanes:
        w, b = snap[wname][h].copy(), np.float32(snap[bname][h])
        for s0 in range(0, len(slots[wname, h]), step):
            accw, accb = np.zeros_like(w), np.float32(0.0)
            for q, i in slots[wname, h][s0:s0 + step]:
                priv, pw, pb = before[q, 0]
                st = {name: v.copy() for name, v in snap.items()}
                st["W_user"][priv] = pw
                st["u_bias"][priv] = pb
                for r in range(len(spans_[q])):   # the span from its start; the rows after i only close the port's span
                    reset_shared(st)
                    if r == i:
                        _, bw, bb = before[q, i]
                        assert np.array_equal(st["W_user"][priv].view(np.uint32), bw.view(np.uint32)), "the replay left the walk's private row"
                        assert np.float32(st["u_bias"][priv]).view(np.uint32) == bb.view(np.uint32), "the replay left the walk's private bias"
                        st[wname][h] = w
                        st[bname][h] = b
                    _set(o, st)
                    feed(q, r)
                    if r == i:
                        accw = (accw + (o.view(wname)[h] - w).astype(np.float32)).astype(np.float32)
                        if with_bias:
                            accb = np.float32(accb + np.float32(np.float32(o.view(bname)[h]) - b))
                    st["W_user"][priv] = o.view("W_user")[priv]
                    st["u_bias"][priv] = o.view("u_bias")[priv]
            w = (w + accw).astype(np.float32)
            if with_bias:
                b = np.float32(b + accb)
        out[wname][h] = w
        out[bname][h] = b
    _set(o, out)
    return len(uhot), len(ihot)


def step_rows(o, d, B, *, fu=(), fi=(), sub=0, isub=0, user_bias=True, hot_over=None, ihot_over=None):
    """one window (CSRData d, rows in file order) on oracle trainer o, which has loaded the tables fu / fi (read_table of its files)"""
    _window(o, B, [[row] for row in _rows(d, B, fu, fi)], lambda q, r: o.update_csr(*d.row(q)), sub, isub, user_bias, hot_over, ihot_over)


def step_blocks(o, blocks, B, *, sub=0, isub=0, user_bias=True, hot_over=None, ihot_over=None):
    """one window (PlusBlocks in file order, every span closed) on the user-group oracle trainer o (B = num_user: no shared rows); returns
    (hot user rows, hot item rows)"""
    def tag(n, r):
        return TAG_DEFAULT if n == 1 else TAG_START if r == 0 else TAG_END if r == n - 1 else TAG_MIDDLE

    sp = spans(blocks)
    fed = [[PlusBlock(*((fbi, fbv) if tag(d.num_row, r) != TAG_MIDDLE else EMPTY), d.slice_rows(r, r + 1), tag(d.num_row, r))
            for r in range(d.num_row)] for fbi, fbv, d in sp]
    return _window(o, B, [_rows(d, B, fids=[int(x) for x in fbi]) for fbi, _, d in sp], lambda q, r: o.update_block(fed[q][r]),
                   sub, isub, user_bias, hot_over, ihot_over)


def row_cuts(n, W):
    """the window sequence's cuts (svdf_wseq.cpp: wseq_from_csr): window w = rows [n w / W, n (w + 1) / W)"""
    return [(n * w // W, n * (w + 1) // W) for w in range(W)]


def block_cuts(ba, W):
    """the block sequence's cuts (svdf_wseq_rule.h: wseq_block_cuts): even block positions moved forward to where no span is open"""
    nb, tag = ba.num_block, ba.extend_tag
    cut = [0]
    for w in range(1, W):
        pos = max(nb * w // W, cut[-1])
        while 0 < pos < nb and tag[pos - 1] in (TAG_START, TAG_MIDDLE):
            pos += 1
        cut.append(pos)
    cut.append(nb)
    return list(zip(cut[:-1], cut[1:]))


def simulate_rows(o, d, B, W, passes, **kw):
    """`passes` passes over the rows of d in W windows; kw: step_rows'.  Returns o"""
    for _ in range(passes):
        for b0, b1 in row_cuts(d.num_row, W):
            step_rows(o, d.slice_rows(b0, b1), B, **kw)
    return o


def simulate_blocks(o, ba, B, W, passes, cuts=None, **kw):
    """`passes` passes over the block sequence in W windows (or the given cuts); kw: step_blocks'.  Returns the hot rows applied
    (user rows, item rows): the library's counters 35 and 36"""
    blocks = ba.to_blocks()
    nu, ni = 0, 0
    for _ in range(passes):
        for b0, b1 in (cuts or block_cuts(ba, W)):
            a, b = step_blocks(o, blocks[b0:b1], B, **kw)
            nu, ni = nu + a, ni + b
    return nu, ni


# ---- draws

def random_table(rng, num_rows, lo, hi, max_children=2, p_none=0.2, vals=(1.0, 0.5, 0.25, 2.0, 0.75), hot=(), hot_p=0.0):
    """per id 0 .. max_children distinct children drawn from [lo, hi) (a feature_user table for amd:shared_user_from = B: lo = B); `hot`
    children are drawn with probability hot_p per id (many slots per window), the rest uniformly (rare ones: applied in place)"""
    rows = []
    for _ in range(num_rows):
        n = 0 if rng.random() < p_none else int(rng.integers(1, max_children + 1))
        n = min(n, hi - lo)
        ch = []
        if n and hot and rng.random() < hot_p:
            ch.append(int(rng.choice(hot)))
        while len(ch) < n:
            x = int(rng.integers(lo, hi))
            if x not in ch:
                ch.append(x)
        rows.append([(c, float(rng.choice(vals))) for c in ch])
    return rows


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


def table_rows(rng, n, num_private, num_shared, num_item, num_global=0, max_g=0, max_shared=2, max_items=1, uvals=False, ivals=False,
               positions=("first", "middle", "last"), hot_items=(), hot_p=0.0):
    """rows of (globals, [private user + 0 .. max_shared shared ids num_private + j], 1 .. max_items distinct items); the private entry
    sits first, in the middle or last of the user section, by `positions`.  ivals: item values other than 1 (the item-side forms of the
    children differ from plain entries only then)"""
    rows = []
    for _ in range(n):
        g = sorted(int(x) for x in rng.choice(num_global, size=int(rng.integers(0, max_g + 1)), replace=False)) if num_global and max_g else []
        ns = min(int(rng.integers(0, max_shared + 1)), num_shared)
        sh = [num_private + int(x) for x in rng.choice(num_shared, size=ns, replace=False)] if ns else []
        sh = [(s, float(rng.choice([1.0, 0.5, 2.0])) if uvals else 1.0) for s in sh]
        priv = (int(rng.integers(0, num_private)), float(rng.choice([1.0, 0.5, 1.5])) if uvals else 1.0)
        pos = str(rng.choice(list(positions)))
        at = 0 if pos == "first" else len(sh) if pos == "last" else (len(sh) + 1) // 2
        users = sh[:at] + [priv] + sh[at:]
        nitem = min(int(rng.integers(1, max_items + 1)), num_item)
        if hot_items and rng.random() < hot_p:
            it = [int(rng.choice(hot_items))]
        else:
            it = [int(rng.integers(0, num_item))]
        while len(it) < nitem:
            x = int(rng.integers(0, num_item))
            if x not in it:
                it.append(x)
        items = [(x, float(rng.choice([1.0, 0.5, -0.75, 1.25])) if ivals else 1.0) for x in it]
        rows.append((float(rng.integers(1, 6)), [(x, float(rng.uniform(0.1, 1.0))) for x in g], users, items))
    return CSRData.from_rows(rows)


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
            blocks.append(PlusBlock(fbi, fbv, d.slice_rows(0, 1), TAG_START))
            blocks.append(PlusBlock(EMPTY[0], EMPTY[1], d.slice_rows(1, nrow - 1), TAG_MIDDLE))
            blocks.append(PlusBlock(fbi, fbv, d.slice_rows(nrow - 1, nrow), TAG_END))
        else:
            blocks.append(PlusBlock(fbi, fbv, d, TAG_DEFAULT))
    return blocks

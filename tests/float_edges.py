"""Models at the edges of float32 -- denormals, exact zeros of both signs, overflow to inf and NaN, saturated sigmoid links -- for the parity
tests of tests/test_float_edges.py (CPU: the inputs are proven on the oracle alone) and tests/test_gpu_float_edges.py (the HIP engine against
the oracle).  Helper module, not collected.

A CASE is one (route shape, stratum, num_factor[, variant]): the config pairs, the training data, and the arrays that go into the model with
set_view after init_trainer.  The data comes from the generators of tests/cases.py at small sizes.  Every model has EXTRA ids per table beyond
the ones the generators draw: untouched rows in most strata, the huge rows and their sinks in `overflow`.

Strata
  denormal        factor rows N(0,1) * 1e-38, biases N(0,1) * 1e-39: products and decayed values land below FLT_MIN
  tiny_mixed      every third row at 1e-38 (biases 1e-39), the rest at 0.01; reg_method = 2 with wd 1e-5 on the lower half of the ids and a DENORMAL
                  wd (1e-40) on the upper half, so project() fires on every 0.01-scale row and divides / takes roots with denormal operands.  The
                  rows of the data keep to one class (ids = 0 mod 3, or the others) except in the last 1 % of a pass, where the classes mix:
                  that is what leaves denormal rows at the end of a pass and still adds denormals to normals
  zeros           rows all +0 (ids = 0 mod 7), rows all -0 (1 mod 7), single -0 elements elsewhere, user_nonnegative = 1, and an L1 threshold
                  (reg_method 1, 3 or 5: variant) with lr * wd sized from the touches per row so that part of the elements is thresholded to 0
                  and part survives.  Two instances pair the all +0 user row `num_user` with an all -0 item row under a negative gradient: the one
                  place where a trained -0 survives (item side decaying by a factor, reg_method 3) and the run from +0 gives other bits
  overflow       four user rows and four item rows among the EXTRA ids at 1e19 .. 1e21, one of them with a +inf element, one item bias -inf; a
                  dozen instances in the last 3 % of every batch pair them with each other (the dot product overflows) and with SINK ids, extra
                  rows of normal scale that no other instance reads, and the last two instances of the pass leak two sinks into ordinary rows.
                  All other rows are at 0.01
  saturated_link  sigmoid links (active_type 1, 2, 3; rank pairs): user rows scaled so that the pre-link sums have a standard deviation of 70,
                  20 or 1 (by id mod 3) -- they cover +-(80 .. 110), both thresholds of expf(-x) and its denormal results
"""
import zlib

import numpy as np

import cases
from oracle import oracle
from svdfeature_amd.multi_gpu import block_window_bounds
from svdfeature_amd.data import BlockArrays, CSRData, PlusBlock, TAG_DEFAULT, TAG_MIDDLE, TAG_START, pairs_as_csr

F = np.float32
FLT_MIN = float(np.finfo(F).tiny)
EXTRA = 8          # ids per table beyond the generators' range: 0..3 special (overflow: huge), 4..7 sinks
STRATA = ("denormal", "tiny_mixed", "zeros", "overflow", "saturated_link")
VIEWS = ("W_user", "W_item", "u_bias", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias")


def same_bits_or_nan(got, want, what=""):
    """NaN sits at the same positions in both arrays, and everywhere else the uint32 patterns are equal: +-0, +-inf, every denormal.

    The bits of a NaN are outside the contract, and only they: the reference on x86 produces the default NaN of SSE for an invalid operation,
    0xffc00000 (inf - inf, 0 * inf), and passes payloads of its operands on, so its models hold 0xffc00000 and 0x7fc00000; the GPU generates
    0x7fc00000 for an invalid operation.  Where a NaN appears, and every bit of every other value, is part of the contract."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, "%s: shapes %s and %s" % (what, got.shape, want.shape)
    g, w = got.ravel(), want.ravel()
    gn, wn = np.isnan(g), np.isnan(w)
    if not np.array_equal(gn, wn):
        at = int(np.flatnonzero(gn != wn)[0])
        raise AssertionError("%s: NaN at different positions (%d here, %d in the reference); first at flat index %d: 0x%08x here, 0x%08x there"
                             % (what, gn.sum(), wn.sum(), at, g.view(np.uint32)[at], w.view(np.uint32)[at]))
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~wn
    if bad.any():
        at = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d values differ in their bits; first at flat index %d: 0x%08x (%r) here, 0x%08x (%r) in the reference"
                             % (what, bad.sum(), bad.size, at, g.view(np.uint32)[at], float(g[at]), w.view(np.uint32)[at], float(w[at])))


def count_different(a, b):
    """values whose bits differ, a NaN on both sides counted as equal"""
    a, b = np.ascontiguousarray(a, F).ravel(), np.ascontiguousarray(b, F).ravel()
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def classes(a):
    """how many values of an array are denormal, +0, -0, +-inf, NaN"""
    a = np.ascontiguousarray(a, F).ravel()
    with np.errstate(invalid="ignore"):
        b = np.abs(a)
        zero = b == 0
        return dict(n=a.size, denormal=int(((b > 0) & (b < FLT_MIN)).sum()), pos_zero=int((zero & ~np.signbit(a)).sum()),
                    neg_zero=int((zero & np.signbit(a)).sum()), pos_inf=int((a == np.inf).sum()), neg_inf=int((a == -np.inf).sum()),
                    nan=int(np.isnan(a).sum()), finite=int(np.isfinite(a).sum()))


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """what a (shape, stratum, k, variant) stands for; `batches` is the pass in file order: ("triples", u, i, r), ("pairs", u, p, q),
    ("rows", CSRData) or ("blocks", [PlusBlock])"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def csr(self, b):
        if b[0] == "triples":
            return CSRData.from_triples(b[1], b[2], b[3])
        if b[0] == "pairs":
            return pairs_as_csr(b[1], b[2], b[3])
        assert b[0] == "rows"
        return b[1]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _late(n, m, tail=0.03):
    """m insertion points, in order, inside the last `tail` of a batch of n (positions in the batch BEFORE the insertion)"""
    lo = int(n * (1.0 - tail))
    return [lo + (n - lo) * j // m for j in range(m)]


def _insert_rows(d, at, rows):
    """CSRData d with rows[j] (a CSRData of one row) put before position at[j]"""
    parts, prev = [], 0
    for pos, row in zip(at, rows):
        parts += [d.slice_rows(prev, pos), row]
        prev = pos
    parts.append(d.slice_rows(prev, d.num_row))
    return CSRData.concat(parts)


def _one_class(ids, tiny, n):
    """ids moved into one class: multiples of 3 (the tiny rows) or the others"""
    ids = np.asarray(ids, np.int64)
    if tiny:
        return ids - ids % 3
    moved = np.where(ids + 1 < n, ids + 1, ids - 1)
    return np.where(ids % 3 == 0, moved, ids)


def _split_classes(b, nu, ni, mix):
    """tiny_mixed: every instance (mix: before the last 1 % of the batch) reads rows of one class only (the class of its first user id)"""
    share = 0.99 if mix else 1.0
    if b[0] in ("triples", "pairs"):
        cols = [np.array(c).astype(np.int64) for c in b[1:]]
        n = len(cols[0])
        head = np.arange(n) < int(n * share)
        tiny = cols[0] % 3 == 0
        for c in range(1, 2 if b[0] == "triples" else 3):
            moved = np.where(tiny, _one_class(cols[c], True, ni), _one_class(cols[c], False, ni))
            cols[c] = np.where(head, moved, cols[c])
        if b[0] == "pairs":   # (pos != neg must survive the move)
            same = cols[1] == cols[2]
            cols[2] = np.where(same, (cols[2] + 3) % (ni - ni % 3), cols[2])
            return ("pairs", cols[0].astype(np.uint32), cols[1].astype(np.uint32), cols[2].astype(np.uint32))
        return ("triples", cols[0].astype(np.uint32), cols[1].astype(np.uint32), b[3])
    assert b[0] == "rows"
    d = b[1]
    idx = d.feat_index.astype(np.int64).copy()
    for r in range(int(d.num_row * share)):
        p = d.row_ptr[3 * r:3 * r + 4]
        tiny = p[2] > p[1] and idx[p[1]] % 3 == 0
        idx[p[1]:p[2]] = _one_class(idx[p[1]:p[2]], tiny, nu)
        idx[p[2]:p[3]] = _one_class(idx[p[2]:p[3]], tiny, ni)
    return ("rows", CSRData(d.row_label, d.row_ptr, idx.astype(np.uint32), d.feat_value))


def _split_block_classes(b, ni, mix):
    """tiny_mixed on user blocks: a user's items and feedback ids take the class of the user (mix: except in the last 1 % of the blocks); two
    feedback ids that the move makes equal are listed once, the values stay n^-1/2"""
    blocks, cut = [], int(len(b[1]) * (0.99 if mix else 1.0))
    while 0 < cut < len(b[1]) and b[1][cut - 1].extend_tag in (TAG_START, TAG_MIDDLE):   # (a START .. END span keeps one feedback list)
        cut += 1
    for j, blk in enumerate(b[1]):
        d = blk.data
        if j >= cut or d.num_row == 0:
            blocks.append(blk)
            continue
        tiny = int(d.feat_index[d.row_ptr[1]]) % 3 == 0
        idx = d.feat_index.astype(np.int64).copy()
        for r in range(d.num_row):
            p = d.row_ptr[3 * r:3 * r + 4]
            idx[p[2]:p[3]] = _one_class(idx[p[2]:p[3]], tiny, ni)
        fb = np.unique(_one_class(blk.index_ufeedback, tiny, ni)).astype(np.uint32) if blk.num_ufeedback else blk.index_ufeedback
        blocks.append(PlusBlock(fb, np.full(len(fb), 1.0 / np.sqrt(max(len(fb), 1)), F), CSRData(d.row_label, d.row_ptr, idx.astype(np.uint32), d.feat_value),
                                blk.extend_tag))
    return ("blocks", blocks)


def _distinct_ids(d):
    """the rows of a CSRData in which no user id and no item id stands twice in its section (what the few-row kernel takes)"""
    keep = np.zeros(d.num_row, bool)
    for r in range(d.num_row):
        _, g, u_, i_, idx, _v = d.row(r)
        keep[r] = len(set(idx[g:g + u_])) == u_ and len(set(idx[g + u_:])) == i_
    return d.select_rows(keep)


def _tail(nu, ni):
    """overflow: the (user, item) instances that touch the special rows (ids nu .. nu+3, ni .. ni+3) -- against sinks (nu+4 .., ni+4 ..), and
    special against special, where the dot product overflows -- and the two that leak a sink into an ordinary row at the end of the pass"""
    su, ku, si, ki = [nu + j for j in range(4)], [nu + 4 + j for j in range(4)], [ni + j for j in range(4)], [ni + 4 + j for j in range(4)]
    first = [(su[0], ki[0]), (ku[0], si[0]), (su[1], si[1]), (su[2], ki[1]), (ku[1], si[2]), (su[3], ki[2]), (ku[2], si[3])]
    return first + first[:5], [(ku[0], 1), (1, ki[0])]


def _add_late(b, tail, leak, ni, ng, label, last, feedback=True):
    """the batch with the instances `tail` spread over its last 3 % and, in the last batch of a pass, `leak` at its very end"""
    spare = ni + 7   # a sink item no instance of `tail` reads first: the second item of a pair / of a two-item row
    if b[0] in ("triples", "pairs"):
        cols = [np.asarray(c) for c in b[1:]]
        n = len(cols[0])
        at = _late(n, len(tail)) + ([n, n] if last else [])
        inst = tail + (leak if last else [])
        new = [np.array([x[0] for x in inst], np.uint32)]
        if b[0] == "triples":
            new += [np.array([x[1] for x in inst], np.uint32), np.full(len(inst), label, F)]
        else:
            new += [np.array([x[1] for x in inst], np.uint32), np.array([spare if x[1] != spare else ni + 6 for x in inst], np.uint32)]
        return (b[0],) + tuple(np.insert(c, at, v).astype(c.dtype) for c, v in zip(cols, new))
    if b[0] == "rows":
        inst = tail + (leak if last else [])
        rows = [CSRData.from_rows([(label, [(ng, 0.5)] if ng is not None and j % 2 else [], [(u, 1.0)], sorted([(i, 1.0), (spare, -0.5)]) if j % 3 == 0 and i != spare else [(i, 1.0)])])
                for j, (u, i) in enumerate(inst)]
        n = b[1].num_row
        return ("rows", _insert_rows(b[1], _late(n, len(tail)) + ([n, n] if last else []), rows))
    assert b[0] == "blocks"
    blocks = list(b[1])
    inst = tail + (leak if last else [])
    new = [PlusBlock(np.array([ni + 4 + j % 2] if feedback else [], np.uint32), np.ones(1 if feedback else 0, F), CSRData.from_rows([(label, [], [(u, 1.0)], [(i, 1.0)]), (label, [], [(u, 1.0)], [(spare, 1.0)])]), TAG_DEFAULT)
           for j, (u, i) in enumerate(inst)]
    n = len(blocks)
    at = []
    for pos in _late(n, len(tail)):   # (never inside a user's START .. END span)
        while pos < n and blocks[pos - 1].extend_tag in (TAG_START, TAG_MIDDLE):
            pos += 1
        at.append(pos)
    for pos, blk in reversed(list(zip(at + ([n, n] if last else []), new))):
        blocks.insert(pos, blk)
    return ("blocks", blocks)


SHAPES = {   # name: (format_type, num_user, num_item, num_global) -- the ids the generators draw; the model has EXTRA more per table
    "staged": (0, 60, 45, 5), "triples": (0, 300, 200, 0), "hot": (0, 400, 30, 0), "fewrow": (0, 400, 150, 40),
    "pairs": (0, 300, 120, 0), "pairs_by_user": (0, 300, 120, 0), "blocks": (1, 300, 250, 0), "nested": (1, 90, 60, 0),
    "rows_globals": (0, 400, 100, 30), "big": (0, 50000, 5000, 0),
}


def _batches(shape, k, binary):
    fmt, nu, ni, ng = SHAPES[shape]
    bl = (lambda r: (r > 3).astype(F)) if binary else (lambda r: r)
    if shape == "staged":     # the shape of test_every_factor_width_basic_and_general
        u, i, r = cases.planted_triples(3000, nu, ni, seed=k)
        return [("triples", u, i, bl(r)), ("rows", cases.sparse_feature_rows(400, nu, ni, ng, seed=100 + k, binary_label=binary))]
    if shape == "triples":
        u, i, r = cases.planted_triples(4000, nu, ni, seed=k)
        return [("triples", u, i, bl(r))]
    if shape == "hot":        # a few items with hundreds of ratings each: runs of a hot row
        u, i, r = cases.planted_triples(5000, nu, ni, seed=k, zipf=True)
        return [("triples", u, i, bl(r))]
    if shape == "fewrow":     # at most two user and two item ids per row, no id twice in a section, globals
        d = cases.sparse_feature_rows(3000, nu, ni, ng, seed=k + 1, max_g=4, max_u=2, max_i=2, allow_dup=False, binary_label=binary)
        return [("rows", _distinct_ids(d))]
    if shape in ("pairs", "pairs_by_user"):
        u, p, q = cases.planted_pairs(4000, nu, ni, seed=k)
        if shape == "pairs_by_user":   # the generator's own order: a user's pairs back to back
            o = np.argsort(u, kind="stable")
            u, p, q = u[o], p[o], q[o]
        return [("pairs", u, p, q)]
    if shape == "big":        # 2^20 ratings: what the default routing of plain ratings takes for the runs pass
        u, i, r = cases.planted_triples(1 << 20, nu, ni, seed=k)
        return [("triples", u, i, bl(r))]
    if shape == "rows_globals":   # one user entry per row (values 1 or 0.5), 0 .. 4 global entries, sometimes a second item entry of value -1:
        rng = np.random.default_rng(k)   # the ragged rows of the window step's own test (tests/test_gpu_wunit.py)
        rows = []
        for _ in range(3000):
            gl = [(int(g), float(rng.uniform(0.1, 1.0))) for g in sorted(rng.choice(ng, size=int(rng.integers(0, 5)), replace=False))]
            items = [(int(rng.integers(0, ni)), 1.0)]
            if rng.random() < 0.3:
                x = int(rng.integers(0, ni))
                if x != items[0][0]:
                    items = sorted(items + [(x, -1.0)])
            rows.append((float(rng.integers(0, 2) if binary else rng.integers(1, 6)), gl, [(int(rng.integers(0, nu)), float(rng.choice([1.0, 0.5])))], items))
        return [("rows", CSRData.from_rows(rows))]
    if shape == "blocks":
        return [("blocks", cases.user_blocks(220, nu, ni, ni, seed=k, max_rows=12, max_fb=10, split_every=6, binary_label=binary))]
    assert shape == "nested"
    return [("blocks", cases.nested_blocks(60, nu, ni, ni, seed=k))]


_cases = {}


def case(shape, stratum, k, variant=None):
    """the Case of a route shape, a stratum and a width; variant: zeros -> reg_method (1, 3, 5; default 3), tiny_mixed -> reg_method (2, 4;
    default 2), saturated_link -> active_type (1, 2, 3; default 2; rank pairs always train with 3)"""
    key = (shape, stratum, k, variant)
    if key in _cases:
        return _cases[key]
    fmt, nu, ni, ng = SHAPES[shape]
    pairs = shape.startswith("pairs")
    active = 3 if pairs else 0
    if stratum == "saturated_link":
        active = 3 if pairs else (variant or 2)
    binary = active != 0
    batches = _batches(shape, k, binary and not pairs)
    nfb = ni if fmt == 1 else 0
    if pairs:
        conf = cases.conf_with(cases.PAIR_CONF, learning_rate=0.01)
    else:
        conf = cases.conf_with(cases.BASICMF_CONF, learning_rate=0.01, wd_user_bias=0.001, wd_item_bias=0.001)
        if binary:
            conf = cases.conf_with(conf, base_score=0.5)
    conf = cases.conf_with(conf, num_user=nu + EXTRA, num_item=ni + EXTRA, num_global=ng + 1 if ng else 0, num_factor=k, active_type=active)
    if ng:
        conf = cases.conf_with(conf, wd_global=0.003)
    if fmt == 1:
        conf = cases.conf_with(conf, num_ufeedback=nfb + EXTRA, wd_ufeedback=0.004, wd_ufeedback_bias=0.002, scale_lr_ufeedback=0.7, format_type=1)
    extend = 2 if shape == "nested" else 0
    nrow = sum(sum(x.data.num_row for x in b[1]) if b[0] == "blocks" else b[1].num_row if b[0] == "rows" else len(b[1]) for b in batches)
    # ---- the stratum's config and data
    if stratum == "tiny_mixed":
        conf = cases.conf_with(conf, reg_method=variant or 2, wd_user=1e-5, wd_item=1e-5)
        if variant == 4 and ng:
            conf = cases.conf_with(conf, reg_global=4)
        conf += [("up:wd", "1e-5"), ("up:bound", str(nu // 2)), ("up:wd", "1e-40"), ("up:bound", str(nu + EXTRA)),
                 ("ip:wd", "1e-5"), ("ip:bound", str(ni // 2)), ("ip:wd", "1e-40"), ("ip:bound", str(ni + EXTRA))]
        batches = [_split_block_classes(b, ni, mix=(j == len(batches) - 1)) if b[0] == "blocks" else _split_classes(b, nu, ni, mix=(j == len(batches) - 1))
                   for j, b in enumerate(batches)]
        if shape == "fewrow":   # (a move may put an id twice into a section)
            batches = [("rows", _distinct_ids(b[1])) for b in batches]
    elif stratum == "zeros":
        reg = variant or 3
        # the threshold an item row meets over a pass ~ 0.9 of its elements' scale: lr * wd per touch -- times 2^32 with the lazy form (5), whose
        # instance count since the row's last touch is an unsigned difference taken the other way round (reg_user / reg_item, apex_svd_base.h:211-283)
        wd = 0.9 * 0.01 / (0.01 * 1.3 * nrow / ni) / (2.0 ** 32 if reg == 5 else 1.0)
        conf = cases.conf_with(conf, reg_method=reg, user_nonnegative=1, wd_user="%.4g" % wd, wd_item="%.4g" % wd)
        if reg == 5 and ng:
            conf = cases.conf_with(conf, reg_global=5, wd_global=0.0005)
        # a -0 that survives a touch: the all -0 item row ni + 7 meets the all +0 user row nu twice, with a negative gradient (label 1 against a
        # prediction near 3; of a rank pair it is the negative item): -0 + lr * err * (+0) = -0 + -0 stays -0 where the item side decays by a
        # factor (reg_method 3), and is +0 where the run starts from +0.  An L1 threshold on the item side (1, 5) writes +0 in both runs.
        rare = [(nu, ni + 6 if pairs else ni + 7)] * 2
        batches = [_add_late(b, rare, [], ni, None, 1.0, last=False, feedback=False) for b in batches]
    elif stratum == "overflow":
        label = 1.0 if binary or pairs else 3.0
        tail, leak = _tail(nu, ni)
        batches = [_add_late(b, tail, leak, ni, ng if ng else None, label, last=(j == len(batches) - 1)) for j, b in enumerate(batches)]
    c = Case(shape=shape, stratum=stratum, k=k, variant=variant, fmt=fmt, active=active, extend=extend, conf=conf, batches=batches,
             nu=nu, ni=ni, ng=ng, nfb=nfb, pairs=pairs, key=key)
    c.model = _model(c)
    _cases[key] = c
    return c


def fresh(c, mk, model=None, conf=(), knobs=()):
    """a trainer of mk(format_type, active_type, extend_type) set up for the case: config, init, knobs, the arrays"""
    t = mk(c.fmt, c.active, c.extend)
    t.seed(7)
    for name, v in list(c.conf) + list(conf):
        t.set_param(name, v)
    t.init_model()
    t.init_trainer()
    for name, v in knobs:
        t.set_knob(name, v)
    for name, a in (c.model if model is None else model).items():
        t.set_view(name, a)
    return t


def _port(f, a, e):
    return oracle.OracleTrainer("port", f, a, e)


def _model(c):
    probe = fresh(c, _port, model={})
    shapes = {}
    for name in VIEWS:
        v = probe.view(name)
        if v is not None and v.size:
            shapes[name] = v.shape
    probe.close()
    rng = np.random.default_rng(_seed("model", c.key))
    m = {}
    ordinary = {"W_user": c.nu, "u_bias": c.nu, "W_item": c.ni, "i_bias": c.ni, "g_bias": c.ng, "W_ufeedback": c.nfb, "ufeedback_bias": c.nfb}
    for name, shp in shapes.items():
        z = rng.standard_normal(shp).astype(F)
        w = name.startswith("W_")
        a = z * F(0.01)
        if c.stratum == "denormal":
            a = z * F(1e-38 if w else 1e-39)
        elif c.stratum == "tiny_mixed":
            a[::3] = z[::3] * F(1e-38 if w else 1e-39)
        elif c.stratum == "zeros":
            if w:
                a[rng.random(shp) < 0.06] = F(-0.0)
            a[0::7] = F(0.0)
            a[1::7] = F(-0.0)
            if name == "W_user":
                a[c.nu] = F(0.0)
            if name == "W_item":
                a[c.ni + 7] = F(-0.0)
        elif c.stratum == "overflow":
            n0 = ordinary[name]
            if name == "W_user":
                a[n0 + 0], a[n0 + 1], a[n0 + 3] = z[n0 + 0] * F(1e19), z[n0 + 1] * F(1e21), z[n0 + 3] * F(1e20)
                a[n0 + 2, 1 % shp[1]] = np.inf
            elif name == "W_item":
                a[n0 + 0], a[n0 + 1], a[n0 + 3] = z[n0 + 0] * F(1e19), z[n0 + 1] * F(1e20), z[n0 + 3] * F(1e21)
            elif name == "i_bias":
                a[n0 + 2] = -np.inf
        elif c.stratum == "saturated_link":
            if name == "W_user":
                a = z * (np.array([70.0, 20.0, 1.0], F)[np.arange(shp[0]) % 3] / F(np.sqrt(shp[1])))[:, None]
            elif name == "W_item":
                a = z
        m[name] = np.ascontiguousarray(a, F)
    return m


def model_without_negative_zeros(c):
    """zeros: the same arrays with every -0 replaced by +0"""
    return {name: np.where(a == 0, F(0.0), a).astype(F) for name, a in c.model.items()}


def model_without_huge_rows(c):
    """overflow: the same arrays with the special rows at the scale of all others"""
    rng = np.random.default_rng(_seed("small", c.key))
    out = {}
    for name, a in c.model.items():
        a = a.copy()
        with np.errstate(invalid="ignore"):
            big = ~(np.abs(a) < 1.0)
        a[big] = (rng.standard_normal(int(big.sum())) * 0.01).astype(F)
        out[name] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- runs
def train(t, c, passes=1):
    """the pass, batch by batch, through the staged calls (both the oracle and the HIP trainer have them)"""
    for _ in range(passes):
        for b in c.batches:
            if b[0] == "blocks":
                for blk in b[1]:
                    t.update_block(blk)
            else:
                t.update_batch(c.csr(b))
            t.finish_round()   # (the engine trains what it has staged: each batch reaches the kernel its own rows select)


def train_windows(o, c, windows, sub=0, passes=1, bf16=False):
    """the one-GPU window step on the oracle's checker steps: every batch in `windows` equal windows; a window's rows are the reference's
    update_inner against the window-start item side, whose changes are summed in file order and added once (sub = 0), or move in ordered
    sub-steps of at most `sub` rows per item (svdo_update_window_substeps)"""
    o.set_stale_rounding(bf16)
    for _ in range(passes):
        for b in c.batches:
            if b[0] == "blocks":
                cut = block_window_bounds(BlockArrays.from_blocks(b[1]), windows)   # (even block positions, moved past open START .. END spans)
                for w in range(windows):
                    delta = o.stale_delta_zero()
                    part = b[1][cut[w]:cut[w + 1]]
                    for blk in part:
                        delta = o.update_block_stale(blk, delta)
                    items = np.unique(np.concatenate([_section_ids(blk.data, 2) for blk in part]))
                    fb = np.unique(np.concatenate([blk.index_ufeedback for blk in part]))
                    _add(o, ("W_item", "i_bias", "g_bias", "W_ufeedback", "ufeedback_bias"), delta,
                         {"W_item": items, "i_bias": items, "W_ufeedback": fb, "ufeedback_bias": fb})
                continue
            d = c.csr(b)
            for w in range(windows):   # (the engine cuts n rows into W windows at the positions n w / W)
                win = d.slice_rows(d.num_row * w // windows, d.num_row * (w + 1) // windows)
                if sub:
                    o.update_window_substeps(win, sub)
                else:
                    items = _section_ids(win, 2)
                    _add(o, ("W_item", "i_bias", "g_bias"), o.update_batch_stale(win), {"W_item": items, "i_bias": items, "g_bias": _section_ids(win, 0)})


def _section_ids(d, sec):
    """the distinct ids of section `sec` (0 global, 1 user, 2 item) over all rows of a CSRData"""
    p = d.row_ptr.astype(np.int64)
    lo, hi = p[sec:-1:3], p[sec + 1::3]
    return np.unique(np.concatenate([d.feat_index[a:b] for a, b in zip(lo, hi)] + [np.zeros(0, np.uint32)]))


def _add(o, names, delta, touched):
    """the window's sums added to the rows the window trained; a row without an instance in the window keeps its bits (a -0 stays -0), as
    it does in the reference, which never writes to a row it does not train"""
    for name, dv in zip(names, delta):
        v = o.view(name)
        ids = touched.get(name)
        if v is not None and v.size and ids is not None and len(ids):
            with np.errstate(all="ignore"):
                v[ids] = v[ids] + dv.reshape(v.shape)[ids]
            o.set_view(name, v)


def scores(t, c):
    """the predictions of every row of the pass on the trainer's model, in file order (blocks: the DEFAULT blocks, predict_block's domain)"""
    out = []
    for b in c.batches:
        if b[0] == "blocks":
            out += [t.predict_block(blk) for blk in b[1] if blk.extend_tag == TAG_DEFAULT or c.extend == 2]
        else:
            out.append(t.predict_batch(c.csr(b)))
    return np.concatenate(out)


def collect(t, c):
    out = {name: t.view(name).copy() for name in c.model}
    out["pred"] = scores(t, c)
    return out


_results = {}


def expected(c, how="exact", flush=False, model=None, tag=None, **kw):
    """the oracle's result for the case -- the views of the model after the pass and the predictions on it --, computed once per
    (case, how, flush, tag): how = "exact" (the reference's sequential pass) or "windows" (train_windows(**kw))"""
    key = (c.key, how, flush, tag, tuple(sorted(kw.items())))
    if key in _results:
        return _results[key]
    o = fresh(c, _port, model=model)
    if flush:
        o.set_flush(True)
    try:
        if how == "exact":
            train(o, c, **kw)
        else:
            train_windows(o, c, **kw)
        res = collect(o, c)
    finally:
        if flush:
            o.set_flush(False)
    o.close()
    _results[key] = res
    return res


def factors(res):
    """all factor values of a result in one array"""
    return np.concatenate([res[name].ravel() for name in ("W_user", "W_item", "W_ufeedback") if name in res])


def everything(res):
    return np.concatenate([np.asarray(v, F).ravel() for v in res.values()])


# ---------------------------------------------------------------------------------------------------------------- the routes
class Route:
    """one GPU case: the Case's key, how the oracle trains it (how / kw of expected()), and how the HIP engine is driven: mode "staged"
    (update_batch / update_block), "resident" (a data set per batch, train_dataset) or "window" (resident under amd:step = minibatch),
    extra config pairs and knobs, the data set kinds and the counters that prove the route"""

    def __init__(self, name, shape, stratum, k, variant=None, mode="staged", conf=(), knobs=(), kinds=None, counters=(), how="exact", **kw):
        self.name, self.key, self.mode, self.conf, self.knobs, self.kinds, self.counters = name, (shape, stratum, k, variant), mode, conf, knobs, kinds, counters
        self.how, self.kw = how, kw
        v = "" if variant is None else "%s%d" % ({"zeros": "reg", "tiny_mixed": "reg", "saturated_link": "active"}.get(stratum, "v"), variant)
        self.id = "-".join(x for x in (name, stratum + v, "k%d" % k) if x)

    @property
    def case(self):
        return case(*self.key)

    def expected(self):
        return expected(self.case, self.how, **self.kw)


WIDTHS = [1, 3, 4, 5, 16, 17, 33, 64, 100, 256, 257, 300, 513, 1024]   # (300: the wide rows with every stratum)
EVERY = [("denormal", None), ("tiny_mixed", 2), ("zeros", 1), ("zeros", 3), ("overflow", None), ("saturated_link", 1), ("saturated_link", 2), ("saturated_link", 3)]
THREE = [("denormal", None), ("zeros", 3), ("overflow", None)]
OTHERS = [("tiny_mixed", 2), ("saturated_link", 1), ("saturated_link", 2)]   # ... and the two that THREE leaves out, on the resident routes that take their configs
PLAIN = [("runs_exec", 0), ("pivot_exec", 0)]   # plain ratings as one instance per lane group, whatever their number and order
# counters (svdfeature_amd.h): 4 / 5 / 6 launches of the basicMF / general / few-row kernel, 22 / 23 passes over hot-row units / runs, 29 passes over
# rank pairs as user-run units.  ">0" or an exact number


def _staged():
    out = []
    for k in WIDTHS:
        for s, v in (EVERY if k in (5, 64, 300) else [("denormal", None), ("overflow", None)]):
            out.append(Route("staged", "staged", s, k, v, counters=((5, ">0"),) if k > 256 else ((4, ">0"), (5, ">0"))))
    return out


def _resident():
    out = []
    for s, v in THREE + OTHERS:
        out.append(Route("triples", "triples", s, 64, v, "resident", knobs=PLAIN, kinds=[0], counters=((4, ">0"),)))
        if s in ("denormal", "overflow"):   # (the eight-lane form is taken on the plain configuration only: the other strata's configs never reach it)
            out.append(Route("basic_i8_0", "triples", s, 64, v, "resident", knobs=PLAIN + [("basic_i8", 0)], kinds=[0], counters=((4, ">0"),)))
        if (s, v) in OTHERS:   # every stratum through predict_dataset / eval_dataset / predict_block: the few-row and general kernels, SVD++ units
            for fused in (0, 1):
                out.append(Route("use_fused%d" % fused, "fewrow", s, 64, v, "resident", knobs=[("use_fused", fused)], kinds=[2 if fused else 1],
                                 counters=((6, ">0"), (5, 0)) if fused else ((5, ">0"), (6, 0))))
            for simple in (1, 0):
                out.append(Route("blocks_simple%d_helpers8" % simple, "blocks", s, 64, v, "resident", knobs=[("use_simple_units", simple), ("svdpp_helpers", 8)], kinds=[3]))
            continue
        for st in (0, 1):
            out.append(Route("runs_stage%d" % st, "triples", s, 64, v, "resident", knobs=[("runs_min_rows", 0), ("runs_stage", st), ("pivot_exec", 0)],
                             kinds=[10], counters=((23, 1),)) if s != "zeros" else None)   # (the runs pass: reg_method 0 only)
        out.append(Route("pivot", "hot", s, 64, v, "resident", knobs=[("pivot_min", 100), ("runs_exec", 0)], kinds=[9], counters=((22, 1),)) if s != "zeros" else None)
        for fused in (0, 1):
            out.append(Route("use_fused%d" % fused, "fewrow", s, 64, v, "resident", knobs=[("use_fused", fused)], kinds=[2 if fused else 1],
                             counters=((6, ">0"), (5, 0)) if fused else ((5, ">0"), (6, 0))))
        out.append(Route("fewrow_gslots0", "fewrow", s, 64, v, "resident", knobs=[("fewrow_gslots", 0)], kinds=[2], counters=((6, ">0"),)))
        for i16 in (0, 1):
            out.append(Route("fewrow_i16_%d" % i16, "fewrow", s, 128, v, "resident", knobs=[("fewrow_i16", i16)], kinds=[2], counters=((6, ">0"),)))
        for simple, helpers in ((1, 8), (1, 1), (0, 8)):
            out.append(Route("blocks_simple%d_helpers%d" % (simple, helpers), "blocks", s, 64, v, "resident",
                             knobs=[("use_simple_units", simple), ("svdpp_helpers", helpers)], kinds=[3]))
        out.append(Route("imfb", "nested", s, 16, v, "resident", kinds=[4]))
        # (the staged imfb kernel has neither a kind nor a launch counter of its own: extend_type 2 has no other trainer, so the instances counted
        # under 0 and the parity with the oracle's nested levels are the proof)
        out.append(Route("imfb_staged", "nested", s, 16, v, "staged", counters=((0, "rows"),)))
    for s, v in THREE + [("saturated_link", 3)]:
        out.append(Route("pairs", "pairs", s, 64, v, "resident", knobs=[("pair_units", 0)], kinds=[2], counters=((6, ">0"),)))
        for units in (0, 1):
            out.append(Route("pair_units%d" % units, "pairs_by_user", s, 64, v, "resident", knobs=[("pair_units", units)], kinds=[11 if units else 2],
                             counters=((29, 1 if units else 0),)))
    # 2^20 ratings under the default knobs: the runs pass (basic_i8 = 1 is one of its conditions), eight lanes per row
    out.append(Route("rows_2p20", "big", "denormal", 64, None, "resident", kinds=[10], counters=((23, 1),)))
    return [r for r in out if r is not None]


def _lazy():
    out = []
    for s, v in (("zeros", 5), ("tiny_mixed", 4)):
        out.append(Route("lazy_staged", "staged", s, 64, v, "staged", counters=((5, ">0"), (4, 0))))
        out.append(Route("lazy_resident", "staged", s, 64, v, "resident", kinds=[1, 1], counters=((5, ">0"), (4, 0))))
        out.append(Route("lazy_wide", "staged", s, 300, v, "staged", counters=((5, ">0"),)))
    return out


def _window():
    out = []
    for contrib in ("fp32", "bf16"):
        for s, v in THREE:
            for k in (64, 320):
                out.append(Route("window_" + contrib, "triples", s, k, v, "window", conf=[("amd:contrib", contrib)], knobs=[("window_hot_sub", 0)], kinds=[8],
                                 how="windows", windows=4, bf16=contrib == "bf16"))
            out.append(Route("window_pairs_" + contrib, "pairs", s, 64, v, "window", conf=[("amd:contrib", contrib)], kinds=[8],
                             how="windows", windows=4, bf16=contrib == "bf16"))
            out.append(Route("window_rows_" + contrib, "rows_globals", s, 64, v, "window", conf=[("amd:contrib", contrib)], kinds=[8],
                             how="windows", windows=4, bf16=contrib == "bf16"))
            out.append(Route("window_blocks_" + contrib, "blocks", s, 64, v, "window", conf=[("amd:contrib", contrib)], kinds=[8],
                             how="windows", windows=4, bf16=contrib == "bf16"))
    for s, v in THREE:
        out.append(Route("window_hot_sub", "hot", s, 64, v, "window", knobs=[("window_hot_sub", 16)], kinds=[8], how="windows", windows=3, sub=16))
    return out


STAGED, RESIDENT, LAZY, WINDOW = _staged(), _resident(), _lazy(), _window()
ROUTES = STAGED + RESIDENT + LAZY + WINDOW

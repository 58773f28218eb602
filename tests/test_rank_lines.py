"""Live-model ranking for sections with USER lines and trainers with side tables, the parts that need no GPU: the numpy
statement of the effective user row and of the prepared item side that tests/test_gpu_rank_lines.py compares the GPU against, with the wrong
orders a kernel could take by mistake; the conditions on the inputs that test shares (found and asserted here, on the CPU); and every refusal
of the svdf_rank_*_lines calls that is decided before the device, on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from rank_rounding import cluster
from test_gpu_rank_eval import make_sections
from test_rank_eval import host_trainer
from test_rank_feedback import FB_CONF, make_feedback, ptr_of, rule_lists, rule_pos

F32, F64 = np.float32, np.float64
ROW_WRONG = ("scaled_children", "children_first", "ids_first", "fused")       # wrong orders of the user row
ITEM_WRONG = ("fused_bias", "reassoc_bias", "late_cval")                      # ... and of the prepared item side
NU, NI, NFB, NS = 200, 300, 90, 150
LONG, EMPTY = 40, 5                        # the section whose line has 300 ids, the one whose line is empty


# ---- the rule
def snap(a):
    """the reference's scalar_map: a value within 1e-6 of 1 multiplies as exactly 1 (a NaN too: its |a - 1| > 1e-6 test is false)"""
    a = F32(a)
    return a if np.abs(a - F32(1.0)) > F32(1e-6) else F32(1.0)


def axpy(f, row, a, fused=False):
    """f + row * a: product and sum rounded to float32 one at a time, or (wrong) in float64 with one rounding"""
    a = snap(a)
    if fused:
        return (f.astype(F64) + row.astype(F64) * F64(a)).astype(F32)
    return f + row * a


def read_side_table(path):
    """a feature_user / feature_item text table (``n idx:val ...`` per id) as (row_ptr, index, value)"""
    ptr, idx, val = [0], [], []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            for ent in tok[1:1 + int(tok[0])]:
                i, v = ent.split(":")
                idx.append(int(i))
                val.append(F32(float(v)))
            ptr.append(len(idx))
    return np.array(ptr, np.int64), np.array(idx, np.int64), np.array(val, F32)


def children(table, i):
    """(child id, value) pairs of id i in table order; ids at or past the table's rows have none"""
    if table is None or i >= len(table[0]) - 1:
        return []
    return [(int(table[1][c]), table[2][c]) for c in range(table[0][i], table[0][i + 1])]


def rule_line_rows(U, lines, table=None, Wfb=None, fb=None, order="pinned"):
    """the documented rule for user rows: tu = 0, or 0 + sum_j Wfb[fid_j] * val_j in list order; then per entry of the USER line, in line
    order, tu += U[uid] * val and, behind it, tu += U[cid] * cval for the children of uid in table order -- a child is not scaled by val and
    its own children are not followed.  Every product and sum is rounded to float32 on its own; a NaN line (or feedback) value reaches the
    whole row.  Wrong orders: "scaled_children" multiplies the child by cval * val, "children_first" adds the children before their
    parent's row, "ids_first" all line ids and then all children, "fused" every multiply-add in float64 with one rounding."""
    ul_ptr, ul_index, ul_value = lines
    fused = order == "fused"
    rows = np.zeros((len(ul_ptr) - 1, U.shape[1]), F32)
    for s in range(len(ul_ptr) - 1):
        f = np.zeros(U.shape[1], F32)
        if fb is not None:
            for j in range(fb[0][s], fb[0][s + 1]):
                f = axpy(f, Wfb[fb[1][j]], fb[2][j], fused)
                if np.isnan(fb[2][j]):
                    f = f + F32(np.nan)
        ent = [(int(ul_index[j]), F32(ul_value[j])) for j in range(ul_ptr[s], ul_ptr[s + 1])]

        def parent(f, uid, v):
            f = axpy(f, U[uid], v, fused)
            return f + F32(np.nan) if np.isnan(v) else f

        def kids(f, uid, v):
            for cid, cv in children(table, uid):
                f = axpy(f, U[cid], F32(cv * v) if order == "scaled_children" else cv, fused)
            return f

        if order == "ids_first":
            for uid, v in ent:
                f = parent(f, uid, v)
            for uid, v in ent:
                f = kids(f, uid, v)
        else:
            for uid, v in ent:
                f = kids(f, uid, v) if order == "children_first" else f
                f = parent(f, uid, v)
                f = kids(f, uid, v) if order != "children_first" else f
        rows[s] = f
    return rows


def rule_item_side(W, bias, table=None, order="pinned"):
    """the documented rule for the item side: without a table W and bias themselves; with one, per item i,
    f = 0; f += W[i] * 1; per child in table order f += W[cid] * (float)((double)cval * 1.0), and b = 0 + bias[i] * 1; per child
    b = b + bias[cid] * cval * 1 -- one float32 operation at a time.  Wrong orders: "fused_bias" adds bias[cid] * cval with one rounding,
    "reassoc_bias" sums the children's products first and adds that sum to the item's bias, "late_cval" keeps W[cid] * cval as a double
    product and rounds only after the add."""
    if table is None:
        return W, bias
    rows, out = np.zeros_like(W), np.zeros_like(bias)
    for i in range(len(W)):
        f = axpy(np.zeros(W.shape[1], F32), W[i], F32(1.0))
        b = F32(0.0) + bias[i] * F32(1.0)
        side = F32(0.0)
        for cid, cv in children(table, i):
            a = F32(F64(cv) * 1.0)
            f = axpy(f, W[cid], a, fused=order == "late_cval")
            if order == "fused_bias":
                b = F32(F64(b) + F64(bias[cid]) * F64(cv))
            elif order == "reassoc_bias":
                side = side + bias[cid] * cv * F32(1.0)
            else:
                b = b + bias[cid] * cv * F32(1.0)
        rows[i], out[i] = f, (b + side if order == "reassoc_bias" else b)
    return rows, out


def rule_both(c, top_n, order="pinned"):
    """(rank_topn's tuple, (position, tied)) of the sections of c by the rule, `order` naming one wrong order of either side"""
    rows = rule_line_rows(c["U"], c["lines"], c.get("table_u"), c.get("Wfb"), c.get("fb"), order if order in ROW_WRONG else "pinned")
    W, bias = rule_item_side(c["W"], c["bias"], c.get("table_i"), order if order in ITEM_WRONG else "pinned")
    return (rule_lists(rows, W, bias, top_n, c["ban_ptr"], c["ban_item"]),
            rule_pos(rows, W, bias, c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"]))


# ---- tables and lines
def write_hand_table(path, num_ids, seed):
    """a table written by hand: id 0 without children, id 1 with 5, id 2 whose child 3 has a child of its own, id 4 its own child, id 5 with
    a repeated child; then 0 .. 2 random children per id; 40 rows fewer than the id space has ids"""
    rng = np.random.default_rng(seed)
    rows = [[], [(7, 0.5), (8, 0.25), (9, -0.75), (10, 0.3), (11, 0.9)], [(3, 0.6)], [(4, 0.5)], [(4, 0.25)], [(6, 0.3), (6, 0.7)]]
    for _ in range(len(rows), num_ids - 40):
        rows.append([(int(rng.integers(0, num_ids)), float(F32(rng.uniform(0.1, 1.0)))) for _ in range(int(rng.integers(0, 3)))])
    with open(path, "w") as f:
        for r in rows:
            f.write(("%d %s" % (len(r), " ".join("%d:%.9g" % e for e in r))).strip() + "\n")


def make_lines(S, nu, seed, long_at=LONG, empty_at=EMPTY, longest=4):
    """S USER lines.  By s % 5: u:1; three ids with a negative value and 1 +- 5e-7 (which multiply as 1); a repeated id; 1 .. `longest`
    ids with any values; u:1 again.  The first id of the sections below 24 is s % 8 (the rows of write_hand_table); section `long_at` has
    300 ids, section `empty_at` none."""
    rng = np.random.default_rng(seed)
    idx, val = [], []
    for s in range(S):
        kind = s % 5
        if s == empty_at:
            i, v = [], []
        elif s == long_at:
            i, v = rng.integers(0, nu, 300), rng.uniform(-1.0, 1.0, 300)
        elif kind in (0, 4):
            i, v = rng.integers(0, nu, 1), [1.0]
        elif kind == 1:
            i, v = rng.integers(0, nu, 3), [-0.625, 1.0 + 5e-7, 1.0 - 5e-7]
        elif kind == 2:
            i, v = rng.integers(0, nu, 3), rng.uniform(-1.0, 0.95, 3)
            i[2] = i[0]
        else:
            n = int(rng.integers(1, longest + 1))
            i, v = rng.integers(0, nu, n), rng.uniform(-1.0, 0.95, n)
        i = np.array(i, np.uint32)
        if s < 24 and len(i):
            i[0] = s % 8
            if kind == 2:
                i[2] = i[0]
        idx.append(i)
        val.append(np.array(v, F32))
    return ptr_of(idx), np.concatenate(idx), np.concatenate(val)


def unit_lines(users):
    """the lines u:1 of the old calls' sections"""
    users = np.asarray(users, np.uint32)
    return np.arange(len(users) + 1, dtype=np.int64), users, np.ones(len(users), F32)


def section_lists(seed, nu=NU, ni=NI, fb=False):
    _, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(NS, nu, ni, seed=seed)
    c = dict(pos_ptr=pos_ptr, pos_item=pos_item, ban_ptr=ban_ptr, ban_item=ban_item, lines=make_lines(NS, nu, seed + 3))
    if fb:
        c["fb"] = make_feedback(NS, NFB, seed=seed + 7)
    return c


def lines_conf(nu, ni, k, fmt, tables=(), base=cases.BASICMF_CONF):
    """the configuration of a trainer of width k; tables: (key, path) pairs"""
    kw = dict(num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.1)
    if fmt == 1:
        kw.update(FB_CONF)
    return cases.conf_with(base, **kw) + list(tables)


def training_input(k, fmt, ni=NI):
    """one pass: rows with several user and item ids (format_type = 0), or SVD++ user blocks"""
    if fmt == 1:
        return cases.user_blocks(100, NU, ni, NFB, seed=k)
    return cases.sparse_feature_rows(1500, NU, ni, 0, seed=k)


def write_tables(tmp, which, nu=NU, ni=NI):
    """which: "hand" / "generated" (both tables), "user" / "item" (one generated table), "none" -> ((key, path) pairs, table_u, table_i)"""
    fu, fi = str(tmp / "feat_user.txt"), str(tmp / "feat_item.txt")
    pairs = []
    if which == "hand":
        write_hand_table(fu, nu, 11)
        write_hand_table(fi, ni, 12)
    else:
        cases.write_side_table(fu, nu - 5, nu, 13)
        cases.write_side_table(fi, ni, ni, 14)
    if which in ("hand", "generated", "user"):
        pairs.append(("feature_user", fu))
    if which in ("hand", "generated", "item"):
        pairs.append(("feature_item", fi))
    tu = read_side_table(fu) if ("feature_user", fu) in pairs else None
    ti = read_side_table(fi) if ("feature_item", fi) in pairs else None
    return pairs, tu, ti


# ---- the rounding input: clustered item rows and biases (one base +- a few hundred ulp), every item with two children of fixed values, so
# that the prepared rows stay clustered and the scores of a section lie a few ulp apart; user rows of mixed magnitude, lines of 1 .. 6 ids
_rounding = {}
BIAS_BASE = 30.0
ROUNDING_KS = (64, 320)


def rounding_input(k, tmp=None):
    if k not in _rounding:
        nu, ni, S, N = 60, 500, 70, 50
        rng = np.random.default_rng(300 + k)
        W = cluster(rng, ni, k, 800)
        bias = (np.full(ni, F32(BIAS_BASE + rng.standard_normal())).view(np.int32) + rng.integers(-40, 41, ni).astype(np.int32)).view(F32)
        U = (rng.standard_normal((nu, k)) * 10.0 ** rng.uniform(-2, 1, (nu, 1))).astype(F32)
        _, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(S, nu, ni, seed=k + 1, big=10, empty=-1, full_ban=-1, npos_big=150)
        lines = make_lines(S, nu, seed=k + 2, long_at=-1, empty_at=-1, longest=6)
        item_rows = [[(int(rng.integers(0, ni)), 0.37), (int(rng.integers(0, ni)), 0.7319)] for _ in range(ni)]
        user_rows = [[(int(rng.integers(0, nu)), float(F32(rng.uniform(0.1, 1.0)))) for _ in range(int(rng.integers(0, 4)))] for _ in range(nu - 9)]
        _rounding[k] = dict(nu=nu, ni=ni, S=S, N=N, k=k, U=U, W=W, bias=bias, pos_ptr=pos_ptr, pos_item=pos_item, ban_ptr=ban_ptr,
                            ban_item=ban_item, lines=lines, item_rows=item_rows, user_rows=user_rows)
        for name, rows in (("table_u", user_rows), ("table_i", item_rows)):
            n = [len(r) for r in rows]
            _rounding[k][name] = (ptr_of(rows), np.array([e[0] for r in rows for e in r], np.int64), np.array([e[1] for r in rows for e in r], F32))
            assert sum(n) == len(_rounding[k][name][1])
    return _rounding[k]


def write_rounding_tables(c, tmp):
    """the tables of the rounding input as files, (key, path) pairs"""
    out = []
    for key, rows in (("feature_user", c["user_rows"]), ("feature_item", c["item_rows"])):
        path = str(tmp / (key + ".txt"))
        with open(path, "w") as f:
            for r in rows:
                f.write(("%d %s" % (len(r), " ".join("%d:%.9g" % e for e in r))).strip() + "\n")
        out.append((key, path))
    return out


_rounding_results = {}


def rounding_results(k, order):
    if (k, order) not in _rounding_results:
        c = rounding_input(k)
        _rounding_results[(k, order)] = rule_both(c, c["N"], order)
    return _rounding_results[(k, order)]


# ---- the route-agreement input: a model trained by one pass through the pinned port with the tables set
ROUTE_CASES = [(64, 0, "hand", 10), (128, 1, "generated", 100)]      # width, format_type, tables, top_n
_route = {}


def route_input(k, fmt, which, top_n, tmp):
    if k not in _route:
        pairs, tu, ti = write_tables(tmp, which)
        t = oracle.OracleTrainer("port", fmt, 0)
        t.seed(3)
        for kk, v in lines_conf(NU, NI, k, fmt, pairs):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        fresh = t.view("W_user").copy()
        if fmt == 1:
            for b in training_input(k, fmt):
                t.update_block(b)
        else:
            t.update_batch(training_input(k, fmt))
        c = section_lists(k, fb=fmt == 1)
        c.update(U=t.view("W_user").copy(), W=t.view("W_item").copy(), bias=t.view("i_bias").copy(), table_u=tu, table_i=ti, N=top_n, fresh=fresh)
        if fmt == 1:
            c["Wfb"] = t.view("W_ufeedback").copy()
        t.close()
        _route[k] = c
    return _route[k]


def untied_flags(c):
    """(per section: no tie among its top_n + 1 best and at least top_n candidates; per positive: untied), from the rule alone"""
    (_, scores, count, _), (_, tied) = rule_both(c, c["N"] + 1)
    sec = np.array([count[s] >= c["N"] and (np.diff(scores[s, :count[s]]) < 0).all() for s in range(len(count))])
    return sec, tied == 0


# ---- tests of the rule
def test_the_rule_on_a_hand_made_case():
    """small binary fractions (every step exact): an empty line, a repeated id, a negative value, a child that is not scaled by the line's
    value, a child with children of its own, a child equal to its parent, an id past the table"""
    U = np.array([[1, 2, 3, 4], [0.5, 0, -1, 8], [0, 0, 0, 16], [32, 0, 0, 0]], F32)
    table = (np.array([0, 1, 2, 3]), np.array([1, 2, 2]), np.array([0.5, 2.0, 0.25], F32))      # 0 -> 1:0.5, 1 -> 2:2 (not followed from 0), 2 -> 2:0.25
    lines = ([0, 0, 1, 3, 4, 5], [0, 1, 1, 2, 3], np.array([2.0, -1.0, -1.0, 1.0, 0.5], F32))
    want = np.array([[0, 0, 0, 0],
                     [2.25, 4, 5.5, 12],                  # 2 U[0] + 0.5 U[1]: the child is not scaled by 2, its own child not followed
                     [-1, 0, 2, 2 * (-8 + 32)],           # twice (-U[1] + 2 U[2])
                     [0, 0, 0, 20],                       # U[2] + 0.25 U[2]
                     [16, 0, 0, 0]], F32)                 # id 3 is past the table's rows
    for order in ("pinned", "children_first", "ids_first", "fused"):          # exact arithmetic: these orders agree
        np.testing.assert_array_equal(rule_line_rows(U, lines, table, order=order), want)
    assert rule_line_rows(U, lines, table, order="scaled_children")[1].tolist() == [2.5, 4, 5, 16]
    np.testing.assert_array_equal(rule_line_rows(U, lines)[1], 2 * U[0])      # without a table
    Wfb = np.array([[0, 1, 0, 0]], F32)
    got = rule_line_rows(U, lines, table, Wfb, ([0, 1, 1, 1, 1, 1], [0], np.array([4.0], F32)))
    np.testing.assert_array_equal(got, want + np.array([[0, 4, 0, 0]] + [[0] * 4] * 4, F32))
    # the item side: 0 + W[i] * 1, then the children; the bias alike
    W = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], F32)
    bias = np.array([1, 2, 4], F32)
    rows, b = rule_item_side(W, bias, (np.array([0, 2, 2]), np.array([1, 2]), np.array([0.5, -2.0], F32)))
    assert rows.tolist() == [[1, 0.5, 0, -2], [0, 1, 0, 0], [0, 0, 0, 1]] and b.tolist() == [1 + 1 - 8, 2, 4]
    assert rule_item_side(W, bias)[0] is W
    assert not np.signbit(rule_item_side(np.full((1, 4), -0.0, F32), np.array([-0.0], F32), (np.array([0, 0]), np.array([], int), np.array([], F32)))[0]).any()
    # values within 1e-6 of 1 multiply as 1; a NaN value reaches its section's whole row and no other
    near = ([0, 1, 2, 3], [1, 1, 1], np.array([1 + 5e-7, 1 - 5e-7, np.nan], F32))
    rows = rule_line_rows(U, near)
    np.testing.assert_array_equal(rows[:2], U[[1, 1]])
    assert np.isnan(rows[2]).all()


def test_the_lines_and_tables_cover_what_the_issue_names(tmp_path):
    ul_ptr, ul_index, ul_value = make_lines(NS, NU, seed=67)
    n = np.diff(ul_ptr)
    assert n[LONG] == 300 and n[EMPTY] == 0 and (n == 1).sum() > 30 and (n == 3).sum() > 30
    assert any(len(np.unique(ul_index[a:b])) < b - a for a, b in zip(ul_ptr[:-1], ul_ptr[1:]) if b - a == 3)
    assert (ul_value < 0).any() and (ul_value == F32(1 + 5e-7)).any() and (ul_value == F32(1 - 5e-7)).any()
    assert snap(1 + 5e-7) == 1 and snap(1 - 5e-7) == 1 and F32(1 + 5e-7) != 1 and snap(1 + 2e-6) != 1
    assert set(range(8)) <= set(ul_index[ul_ptr[:24]].tolist())          # the rows written by hand are all in use
    path = str(tmp_path / "t.txt")
    write_hand_table(path, NU, 11)
    t = read_side_table(path)
    assert len(t[0]) - 1 == NU - 40 and children(t, 0) == [] and len(children(t, 1)) == 5 and children(t, NU - 1) == []
    assert children(t, 2)[0][0] == 3 and children(t, 3) and children(t, 4)[0][0] == 4 and [c for c, _ in children(t, 5)] == [6, 6]
    assert t[1].max() >= NU - 40                                          # a child past the table's rows


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_the_rounding_input_sees_every_wrong_order(k):
    """conditions on the input tests/test_gpu_rank_lines.py::test_rounding_is_pinned reuses: EVERY wrong order of the user row and of the
    item side changes the top-N list of at least one section and at least one position"""
    c = rounding_input(k)
    (items, _, count, nan), (position, tied) = rounding_results(k, "pinned")
    assert not nan.any() and (count == c["N"]).all()
    n = np.diff(c["lines"][0])
    assert (n > 1).sum() > 20 and (np.abs(c["lines"][2] - 1) > 1e-3).any()
    for wrong in ROW_WRONG + ITEM_WRONG:
        (witems, _, _, _), (wposition, _) = rounding_results(k, wrong)
        assert (witems != items).any(axis=1).sum() >= 1, wrong
        assert (wposition != position).sum() >= 1, wrong


@pytest.mark.parametrize("k, fmt, which, top_n", ROUTE_CASES)
def test_the_route_agreement_input_is_mostly_untied(k, fmt, which, top_n, tmp_path):
    """what the comparison with the CPU ranker relies on: with the oracle trainer on the same training rows at least 90 % of the sections
    have no tie among their top_n + 1 best and at least 90 % of the positives are untied -- and the user rows (children included) have moved"""
    c = route_input(k, fmt, which, top_n, tmp_path)
    sec, pos = untied_flags(c)
    assert sec.mean() >= 0.9 and pos.mean() >= 0.9, (sec.mean(), pos.mean())
    moved = (c["fresh"] != c["U"]).any(axis=1)
    assert moved[np.unique(c["table_u"][1])].any()


# ---- refusals on host-only handles
POS = ([0, 2, 3], [5, 6, 7])
UL = ([0, 1, 3], [3, 19, 4], [1.0, -1.0, 2.0])
FB = ([0, 2, 3], [3, 29, 4], [0.5, -1.0, 2.0])


def calls(t, lines, fb=None):
    """the three methods with one lines argument"""
    return [lambda: t.rank_positions(None, *POS, lines=lines, feedback=fb), lambda: t.rank_eval(None, *POS, lines=lines, feedback=fb),
            lambda: t.rank_topn(None, 5, lines=lines, feedback=fb)]


def group_trainer(ext=0, extra=(), **kw):
    return host_trainer(fmt=1, ext=ext, extra=[("num_ufeedback", 30)] + list(extra), **kw)


def side_tables(tmp_path):
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n0\n2 4:0.25 4:0.5\n")
    return [[], [("feature_user", str(table))], [("feature_item", str(table))], [("feature_user", str(table)), ("feature_item", str(table))]]


def test_a_legal_call_on_a_host_only_handle_needs_a_gpu(tmp_path):
    legal = ([0, 0, 4], [7, 7, 0, 7], [np.nan, -0.0, 1e30, 0.5])         # an empty line, a repeated id, any float value
    for extra in side_tables(tmp_path):
        t0, t1 = host_trainer(extra=extra), group_trainer(1, extra=extra)
        for lines in (UL, legal):
            for call in calls(t0, lines) + calls(t1, lines, FB):
                with pytest.raises(sa.SvdfError, match="rank_(eval|topn) needs a GPU"):
                    call()
        assert t0.counter(41) == t1.counter(41) == 0
        # the old calls on the same handles still refuse the tables
        if extra:
            for call in (lambda: t0.rank_topn([1, 2], 5), lambda: t0.rank_positions([1, 2], *POS), lambda: t1.rank_topn([1, 2], 5, feedback=FB)):
                with pytest.raises(sa.SvdfError, match="rank_(eval|topn): .*side tables change the score"):
                    call()


def test_line_refusals_come_before_the_device():
    t = host_trainer()
    for j, who in enumerate(("rank_eval", "rank_eval", "rank_topn")):       # rank_positions, rank_eval, rank_topn
        call = lambda lines, j=j: calls(t, lines)[j]()
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            call(([0, 1, 3], [3, 20, 4], [1.0, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            call(([0, 1, 3], [3, 4000000000, 4], [1.0, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": ul_ptr must not decrease"):
            call(([0, 3, 2], [3, 19, 4], [1.0, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": ul_ptr must start at >= 0"):
            call(([-1, 1, 3], [3, 19, 4], [1.0, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": ul_ptr is missing"):
            call((None, None, None))
        with pytest.raises(sa.SvdfError, match=who + ": with lines= the sections bring USER lines: users must be None"):
            [t.rank_positions, t.rank_eval, lambda u, *a, **kw: t.rank_topn(u, 5, **kw)][j]([1, 2], *POS, lines=UL)
    # NULL pointers through the C entry points
    ptr, idx, val = np.array(UL[0], np.int64), np.array(UL[1], np.uint32), np.array(UL[2], F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    items, count, nan = np.zeros(10, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    pos_ptr, pos_item, out = np.array(POS[0], np.int64), np.array(POS[1], np.uint32), [np.zeros(3, np.int32) for _ in range(4)]
    for ul_ptr, ul_index, ul_value, msg in ((None, p(idx), p(val), "ul_ptr is missing"), (p(ptr), None, p(val), "ul_index / ul_value is missing"),
                                            (p(ptr), p(idx), None, "ul_index / ul_value is missing")):
        assert t.lib.svdf_rank_topn_lines(t.h, 2, ul_ptr, ul_index, ul_value, None, None, None, None, None, 5, items, None, count, nan) == -1
        assert "rank_topn: " + msg in t.lib.svdf_last_error().decode()
        assert t.lib.svdf_rank_eval_positions_lines(t.h, 2, ul_ptr, ul_index, ul_value, None, None, None, pos_ptr, pos_item, None, None, *out) == -1
        assert "rank_eval: " + msg in t.lib.svdf_last_error().decode()
        m = sa.RankMetrics()
        at = np.array([5], np.int32)
        assert t.lib.svdf_rank_eval_lines(t.h, 2, ul_ptr, ul_index, ul_value, None, None, None, pos_ptr, pos_item, None, None, 1, at, C.byref(m)) == -1
        assert "rank_eval: " + msg in t.lib.svdf_last_error().decode()
    # num_section == 0 is legal and still needs a GPU; the other lists are refused in their own words
    with pytest.raises(sa.SvdfError, match="rank_topn needs a GPU"):
        t.rank_topn(None, 5, lines=([0], [], []))
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions(None, [0, 2, 3], [5, 30, 7], lines=UL)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_topn(None, 257, lines=UL)
    # the feedback triple keeps section 6y's refusals
    g = group_trainer()
    for call in calls(g, UL, None) + calls(g, UL, (None, None, None)):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): fb_ptr is NULL on a user-group trainer.*explicitly as an empty list"):
            call()
    for call in calls(g, UL, ([0, 2, 3], [3, 30, 4], [0.5, -1.0, 2.0])):
        with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
            call()
    for call in calls(g, ([0, 1, 3], [3, 20, 4], [1.0, -1.0, 2.0]), FB):
        with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
            call()
    for call in calls(t, UL, FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): feedback lists need a user-group trainer"):
            call()
    assert t.counter(38) == t.counter(39) == t.counter(41) == g.counter(41) == 0


def test_configuration_refusals_of_the_lines_calls(tmp_path):
    """what the _lines calls still do not cover, in the old calls' words"""
    for ext in (2, 15):
        for call in calls(sa.Trainer(1, 0, ext, device=-2), UL, FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): user-group trainers .*extend_type != 0 are not covered"):
                call()
    for extra in side_tables(tmp_path):
        for call in calls(host_trainer(extra=extra + [("amd:gpus", 2)]), UL) + calls(group_trainer(extra=[("amd:gpus", 2)]), UL, FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): amd:gpus > 1 is not covered"):
                call()
    for call in calls(host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]), UL):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): common_latent_space != 0"):
            call()
    for call in calls(host_trainer(fmt=1, nu=30, extra=[("num_ufeedback", 30), ("common_latent_space", 1), ("common_feedback_space", 1)]), UL, FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): common_latent_space != 0"):
            call()
    with pytest.raises(sa.SvdfError, match="rank_topn: call init_model / load_model and init_trainer first"):
        sa.Trainer(0, 0, 0, device=-2).rank_topn(None, 5, lines=UL)


def test_a_table_with_a_child_outside_its_id_space_is_refused_when_the_trainer_starts(tmp_path):
    """the table loader's own refusal, which the calls repeat once per call (svdf_ranklines_lists.h; tools/check_ranklines_lists.cpp)"""
    table = tmp_path / "feat.txt"
    table.write_text("1 30:0.5\n")
    with pytest.raises(sa.SvdfError, match="feature_item: child index exceed bound"):
        host_trainer(extra=[("feature_item", str(table))])
    with pytest.raises(sa.SvdfError, match="feature_user: child index exceed bound"):
        host_trainer(extra=[("feature_user", str(table))])

"""The rule of svdf_item_topn (include/svdfeature_amd.h) in numpy float32, its decoys, and the inputs the CPU and GPU tests
share (helper of tests/test_item_topn.py and tests/test_gpu_item_topn.py; not collected)."""
import numpy as np

from rank_rounding import dot_fp32
from test_rank_topn import rule_topn

F32 = np.float32
DECOYS = ("reciprocal", "sequential", "double")
METRICS = ("dot", "cosine")


def sum_squares(W, order="pinned"):
    """<W[i], W[i]> per row in float32: the pinned order (four chains, (a0 + a2) + (a1 + a3), the tail) or index order"""
    W = np.ascontiguousarray(W, F32)
    return np.array([dot_fp32(row, row[None, :], order)[0] for row in W], F32) if len(W) else np.zeros(0, F32)


def unit_rows(W, decoy=None):
    """R[i] = W[i] / sqrt(<W[i], W[i]>): the sum of squares in the pinned order, np.sqrt, a divide per element; a sum of 0 gives a +0 row.
    decoy: "reciprocal" multiplies by 1 / n, "sequential" sums the squares in index order, "double" takes the norm in float64, rounded once"""
    W = np.ascontiguousarray(W, F32)
    with np.errstate(all="ignore"):
        ss = sum_squares(W, "sequential" if decoy == "sequential" else "pinned")
        if decoy == "double":
            n = np.sqrt((W.astype(np.float64) ** 2).sum(1)).astype(F32)
            zero = n == 0
        else:
            n = np.sqrt(ss)
            zero = ss == 0
        if decoy == "reciprocal":
            R = W * (F32(1.0) / n)[:, None]
        else:
            R = W / n[:, None]
        R = R.astype(F32)
        R[zero] = F32(0.0)
    return R


def merged_bans(items, ban_ptr, ban_item):
    """every section's ban list with its own query appended"""
    lists = []
    for s, q in enumerate(items):
        b = np.asarray(ban_item[ban_ptr[s]:ban_ptr[s + 1]], np.int64) if ban_ptr is not None else np.zeros(0, np.int64)
        lists.append(np.concatenate([b, [int(q)]]))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return ptr, np.concatenate(lists) if lists else np.zeros(0, np.int64)


def rule_similar(W, items, top_n, metric="cosine", ban_ptr=None, ban_item=None, decoy=None):
    """(items, scores, count, nan) of the documented rule: rule_topn with the base matrix on both sides, a zero bias and the query merged
    into each section's ban list; the base is W for "dot" and the unit rows for "cosine" (`decoy`: one of DECOYS for the unit rows)"""
    W = np.ascontiguousarray(W, F32)
    base = W if metric in ("dot", 0) else unit_rows(W, decoy)
    ptr, ids = merged_bans(items, ban_ptr, ban_item)
    with np.errstate(all="ignore"):
        return rule_topn(base, base, np.zeros(len(W), F32), np.asarray(items, np.int64), top_n, ptr, ids)


def edge_rows(k):
    """the edge rows of the unit-row rule at width k, one per row: zero, -0, denormals whose squares underflow, a denormal norm, a sum of
    squares that overflows, a NaN, an inf"""
    E = np.zeros((7, k), F32)
    E[1] = F32(-0.0)
    E[2] = np.float32(1e-40) * (1 + np.arange(k) % 3)          # squares underflow to 0: the unit row is +0, not W / 0
    E[3] = np.float32(3e-23) * (1 + np.arange(k) % 5)          # the squares are denormal, the norm is not 0
    E[3, 0] = -E[3, 0]
    E[4] = np.float32(2e19) * (1 + np.arange(k) % 2)
    E[4, -1] = -E[4, -1]
    E[4, 0] = F32(3e38)                                        # 9e76 overflows: n = inf, the elements +-0
    E[5] = np.linspace(-1, 1, k, dtype=F32)
    E[5, k // 2] = np.nan
    E[6] = np.linspace(1, 2, k, dtype=F32)
    E[6, 0] = np.inf                                           # inf / inf = NaN in element 0, +0 elsewhere
    return E


def random_rows(n, k, seed):
    return (0.1 * np.random.default_rng(seed).standard_normal((n, k))).astype(F32)


def same_bits(a, b):
    """equal bit for bit, NaN by position (sign and payload of a NaN are not specified)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def pinned_case(k, ni=500, seed=None):
    """the item table of the rounding test at width k: random N(0, 0.1) rows -- the norms differ from row to row, so each decoy of the unit
    rows moves bits -- with a cluster (one base row +- 800 ulp per element, rows 0 .. ni / 2) whose cosine scores lie a few ulp apart"""
    rng = np.random.default_rng(7000 + k if seed is None else seed)
    W = (0.1 * rng.standard_normal((ni, k))).astype(F32)
    base = (0.1 * rng.standard_normal(k)).astype(F32)
    half = ni // 2
    W[:half] = (np.tile(base.view(np.int32), (half, 1)) + rng.integers(-800, 801, (half, k)).astype(np.int32)).view(F32)
    return W

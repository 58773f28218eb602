"""The rule that draws ITEM-WEIGHTED negatives of a pass of rank pairs (include/svdfeature_amd.h), in numpy and Python integers
-- written from the published statement, not from the C++ (helper of tests/test_pair_weight.py and tests/test_gpu_pair_weight.py; not
collected).  The streams are pair_source_rule's.

    cdf[0] = 0, cdf[i + 1] = cdf[i] + item_weight[i], W = cdf[num_item]            1 <= W <= 2^32 - 1
    x(q, t)    = mix(stream_q + (t + 1) * G)                                        all 64 bits
    y          = floor(x * W / 2^64)
    wdraw(q,t) = the item i with cdf[i] <= y < cdf[i + 1]                           bisect_right(cdf, y) - 1
    neg_q      = the first of wdraw(q, 0), wdraw(q, 1), ... not in P(user_r); at most T = 4096 draws
    density    a user with rows is refused when 64 * (W - W(P(u))) < W"""
import bisect

import numpy as np

import pair_source_rule
from rank_negs_rule import G, U64, mix

T = pair_source_rule.T


def cdf_of(item_weight):
    """Python integers [num_item + 1]"""
    out = [0]
    for w in np.asarray(item_weight).tolist():
        out.append(out[-1] + int(w))
    return out


def words(seed, q, t):
    """x(q, t) for arrays of q and t that broadcast: uint64"""
    with np.errstate(over="ignore"):
        return mix(pair_source_rule.stream(seed, q) + (np.asarray(t, U64) + U64(1)) * G)


def lookup(cdf, x):
    """the item of one 64-bit word, in Python integers"""
    y = (int(x) * cdf[-1]) >> 64
    return bisect.bisect_right(cdf, y) - 1


def lookups(cdf, x, exact=False):
    """the items of an array of words.  exact: y in Python integers, word by word.  Otherwise y in uint64 halves -- W < 2^32, so with
    x = xh * 2^32 + xl the product's high 64 bits are (xh * W + ((xl * W) >> 32)) >> 32 and neither term overflows -- which is what the
    large columns of the GPU tests take; test_pair_weight.py holds the two equal on every boundary word.  The inversion is numpy's
    searchsorted on the same cdf."""
    W = cdf[-1]
    flat = np.asarray(x, U64).ravel()
    if exact:
        y = np.array([(int(v) * W) >> 64 for v in flat.tolist()], np.int64)
    else:
        assert 1 <= W <= 0xFFFFFFFF
        y = (((flat >> U64(32)) * U64(W) + (((flat & U64(0xFFFFFFFF)) * U64(W)) >> U64(32))) >> U64(32)).astype(np.int64)
    return (np.searchsorted(np.asarray(cdf, np.int64), y, side="right") - 1).reshape(np.shape(x))


def wdraws(seed, q, t, cdf):
    """wdraw(q, t) for arrays of q and t that broadcast"""
    return lookups(cdf, words(seed, q, t))


def rule_negatives(num_user, num_item, user, pos_item, item_weight, num_neg, seed):
    """uint32[n * num_neg]: what svdf_pair_negatives_weighted returns.  Round t evaluates wdraw(q, t) of every pair still without a negative."""
    cdf = cdf_of(item_weight)
    assert len(cdf) == num_item + 1 and 1 <= cdf[-1] <= 0xFFFFFFFF
    user = np.asarray(user, np.int64)
    n, m = len(user), int(num_neg)
    member = np.zeros((num_user, num_item), bool)
    member[user, np.asarray(pos_item, np.int64)] = True
    pu = np.repeat(user, m)
    neg = np.full(n * m, -1, np.int64)
    open_q = np.arange(n * m)
    for t in range(T):
        if len(open_q) == 0:
            break
        d = wdraws(seed, open_q, t, cdf)
        ok = ~member[pu[open_q], d]
        neg[open_q[ok]] = d[ok]
        open_q = open_q[~ok]
    assert len(open_q) == 0, "pair %d found no negative in %d draws" % (int(open_q[0]), T)
    return neg.astype(np.uint32)


def density_refusal(num_user, user, pos_item, item_weight):
    """None, or (user, held, W) of the first user in id order the weighted density rule refuses"""
    w = np.asarray(item_weight).astype(object)
    W = int(sum(w.tolist()))
    uptr, uitems = pair_source_rule.user_lists(num_user, user, pos_item)
    for u in range(num_user):
        if uptr[u + 1] == uptr[u]:
            continue
        held = int(sum(w[uitems[uptr[u]:uptr[u + 1]].astype(np.int64)].tolist()))
        if 64 * (W - held) < W:
            return u, held, W
    return None


def guide_of(cdf):
    """(log2 Gn, guide[Gn + 1]) of the published guide table"""
    num_item, W = len(cdf) - 1, cdf[-1]
    lg = 6
    while (1 << lg) < num_item:
        lg += 1
    guide = [bisect.bisect_right(cdf, (((g << (64 - lg)) * W) >> 64)) - 1 for g in range(1 << lg)]
    guide.append(max(i for i in range(num_item) if cdf[i + 1] > cdf[i]))
    return lg, guide


def boundary_words(cdf):
    """every boundary word of both tables: for each item of positive weight the smallest x that maps into it and that x - 1; 0 and 2^64 - 1;
    the first and last word of every guide bucket.  uint64, distinct, ascending"""
    num_item, W = len(cdf) - 1, cdf[-1]
    out = {0, (1 << 64) - 1}
    for i in range(num_item):
        if cdf[i + 1] > cdf[i]:
            x = -((-cdf[i] << 64) // W)   # the smallest x with x * W >= cdf[i] * 2^64
            out.add(x)
            if x > 0:
                out.add(x - 1)
    lg = guide_of(cdf)[0]
    for g in range(1 << lg):
        out.add(g << (64 - lg))
        out.add(((g + 1) << (64 - lg)) - 1)
    return np.array(sorted(out), dtype=np.uint64)


# ---- the inputs the CPU and the GPU tests share
PINNED_NI = 1200
NU, NI, N = 200, 300, 3000


def pinned_weights(num_item=PINNED_NI):
    i = np.arange(num_item, dtype=np.int64)
    return np.where(i % 7 == 0, 0, 1 + (i * i) % 97).astype(np.uint32)


def tables():
    """name -> item_weight (uint32): the tables of the lookup tests"""
    full = (1 << 32) - 1
    out = {"pinned": pinned_weights()}
    for ni in (1, 2, 63, 64, 65, 1200, 5000):
        out["ones_%d" % ni] = np.ones(ni, np.uint32)
    heavy = np.ones(1200, np.uint32)
    heavy[417] = full - 1199
    out["one_heavy_full"] = heavy                         # one item holding W - (num_item - 1) of W = 2^32 - 1
    for name, w in (("single_1", 1), ("single_full", full)):
        one = np.zeros(300, np.uint32)
        one[123] = w
        out[name] = one                                   # a single positive item
    z = pinned_weights(5000).copy()
    z[:40] = 0                                            # a zero run at the start,
    z[-75:] = 0                                           # at the end,
    z[2400:2700] = 0                                      # and across guide-bucket edges (Gn = 8192: under one item a bucket)
    out["zero_runs"] = z
    z2 = np.ones(130, np.uint32)
    z2[60:70] = 0                                         # Gn = 256: a zero run across the edge between the buckets around item 64
    out["zero_across_edge"] = z2
    run = np.full(500, 1000, np.uint32)
    run[100:300] = 1
    run[300] = 1 << 31
    out["light_run_heavy"] = run                          # 200 weight-1 items beside one of weight 2^31
    skew = np.zeros(NI, np.uint32)
    skew[:] = 1 + (np.arange(NI, dtype=np.int64) * 37) % 11
    skew[::13] = 0
    out["rows_300"] = skew                                # the table of the 200 x 300 rows below
    return out


def rows(order, n=N, seed=5):
    """pair_hard_rule.rows: n positives of 200 users x 300 items with repeated (user, item) rows"""
    import pair_hard_rule
    return pair_hard_rule.rows(order, n=n, seed=seed)


def row_tables():
    """the tables of 300 items the rows above are drawn under: every one admits them (no user holds 63 / 64 of the weight)"""
    t = tables()
    heavy = np.ones(NI, np.uint32)
    heavy[::3] = 1 << 22
    return {"rows_300": t["rows_300"], "ones_300": np.ones(NI, np.uint32), "heavy_thirds": heavy}

"""The rule that draws the negatives of a pass of rank pairs from a source of positives (include/svdfeature_amd.h), in numpy
uint64 -- written from the published statement, not from the C++.  G and mix are section 6ab's (rank_negs_rule).

    rows r = 0 .. n-1 of (user_r, pos_r);  P(u) = the distinct items of all rows of user u;  num_neg = m negatives per row
    pair q = r * m + j (j = 0 .. m-1) is (user_r, pos_r, neg_q)
    SALT      = 0x70616972736E6567                                   ("pairsneg")
    stream_q  = mix((seed ^ SALT) + (q + 1) * G)
    draw(q,t) = (uint32)(((mix(stream_q + (t + 1) * G) >> 32) * num_item) >> 32)
    neg_q     = the first of draw(q, 0), draw(q, 1), ... that is not in P(user_r); at most T = 4096 draws"""
import numpy as np

from rank_negs_rule import G, U64, mix

SALT = U64(0x70616972736E6567)
T = 4096


def stream(seed, q):
    with np.errstate(over="ignore"):
        return mix((U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ SALT) + (np.asarray(q, U64) + U64(1)) * G)


def draws(seed, q, t, num_item):
    """draw(q, t) for arrays of q and t that broadcast: ids below num_item"""
    with np.errstate(over="ignore"):
        z = mix(stream(seed, q) + (np.asarray(t, U64) + U64(1)) * G)
    return (((z >> U64(32)) * U64(num_item)) >> U64(32)).astype(np.int64)


def user_lists(num_user, user, pos_item):
    """(uptr[num_user + 1], uitems): every user's distinct items, ascending"""
    user, pos_item = np.asarray(user, np.int64), np.asarray(pos_item, np.int64)
    span = int(pos_item.max()) + 1 if len(pos_item) else 1
    key = np.unique(user * span + pos_item)
    uptr = np.zeros(num_user + 1, np.int64)
    np.add.at(uptr, key // span + 1, 1)
    return np.cumsum(uptr), (key % span).astype(np.uint32)


def rule_negatives(num_user, num_item, user, pos_item, num_neg, seed, return_draws=False):
    """uint32[n * num_neg]: what svdf_pair_negatives returns (and, on request, the draws every pair took).  Round t evaluates draw(q, t) of
    every pair still without a negative."""
    user = np.asarray(user, np.int64)
    n, m = len(user), int(num_neg)
    member = np.zeros((num_user, num_item), bool) if num_user * num_item <= (1 << 26) else None
    if member is not None:
        member[user, np.asarray(pos_item, np.int64)] = True
    else:
        sets = {}
        for u, i in zip(user.tolist(), np.asarray(pos_item).tolist()):
            sets.setdefault(u, set()).add(i)
    pu = np.repeat(user, m)
    neg = np.full(n * m, -1, np.int64)
    took = np.zeros(n * m, np.int64)
    open_q = np.arange(n * m)
    for t in range(T):
        if len(open_q) == 0:
            break
        d = draws(seed, open_q, t, num_item)
        if member is not None:
            ok = ~member[pu[open_q], d]
        else:
            ok = np.array([x not in sets[u] for u, x in zip(pu[open_q].tolist(), d.tolist())], bool)
        neg[open_q[ok]] = d[ok]
        took[open_q[ok]] = t + 1
        open_q = open_q[~ok]
    assert len(open_q) == 0, "pair %d found no negative in %d draws" % (int(open_q[0]), T)
    return (neg.astype(np.uint32), took) if return_draws else neg.astype(np.uint32)

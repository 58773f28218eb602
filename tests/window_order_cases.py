"""(not collected by pytest) Inputs in clustered file orders for the window step (`amd:step = minibatch`; svdf_wseq_rule.h: wseq_actual_columns /
wseq_actual_csr).  The window rule sizes its windows from per-pass counts and cuts them at equal positions n w / W; on a
file sorted by item, or one that arrives in bursts, a row's updates do not spread over the windows.  Every generator here returns one seeded
draw in one of these orders:

  shuffled   as generated
  item       stable sort by item id (rank pairs: by the positive item)
  burst      stable sort by item // (ni // 20): 20 blocks of the catalogue, random inside a block
  user       stable sort by user id -- the control: users are walked exactly, their order changes neither the window count nor the accuracy class
  shared     (rows with shared user ids only) stable sort by the shared user id: the same failure on the user side of wseq_from_csr

and tests/window_rule.py's helpers count what the windows as cut hold (what the tests assert the documented bounds on)."""
import numpy as np

import cases
from svdfeature_amd import CSRData
from window_rule import mean_met, window_counts, window_cuts  # noqa: F401  (what the windows as cut hold: counted where the rule is stated)

ORDERS = ("shuffled", "item", "burst", "user")
ROW_ORDERS = ORDERS + ("shared",)
BURST_BLOCKS = 20


def order_of(order, user, item, ni, shared=None):
    """the permutation that puts a draw into `order`"""
    n = len(item)
    if order == "shuffled":
        return np.arange(n)
    key = {"item": lambda: np.asarray(item, np.int64), "burst": lambda: np.asarray(item, np.int64) // max(ni // BURST_BLOCKS, 1),
           "user": lambda: np.asarray(user, np.int64), "shared": lambda: np.asarray(shared, np.int64)}[order]()
    return np.argsort(key, kind="stable")


def triples(n, nu, ni, seed, order, zipf=False):
    u, i, r = cases.planted_triples(n, nu, ni, seed, zipf=zipf)
    p = order_of(order, u, i, ni)
    return u[p], i[p], r[p]


def triples_with_holdout(n, nu, ni, seed, order):
    """n + n // 10 planted ratings, the last tenth (of the draw, before ordering) held out: ((u, i, r) in `order`, (u, i, r) held out)"""
    u, i, r = cases.planted_triples(n + n // 10, nu, ni, seed)
    p = order_of(order, u[:n], i[:n], ni)
    return (u[:n][p], i[:n][p], r[:n][p]), (u[n:], i[n:], r[n:])


def pairs(n, nu, ni, seed, order):
    u, p, q = cases.planted_pairs(n, nu, ni, seed)
    o = order_of(order, u, p, ni)
    return u[o], p[o], q[o]


def shared_rows(n, num_private, num_shared, ni, seed, order):
    """rows of the shape tests/test_gpu_shared_user_window.py trains (_deep_rows): one private user (id < num_private), one shared user id
    num_private + s (an attribute bucket drawn per row, like an item), one item; labels from planted triples.  Returns (CSRData, private user,
    shared id - num_private, item) with the rows in `order`."""
    u, i, r = cases.planted_triples(n, num_private, ni, seed)
    s = np.random.default_rng(seed + 7919).integers(0, num_shared, n).astype(np.uint32)
    p = order_of(order, u, i, ni, s)
    u, i, r, s = u[p], i[p], r[p], s[p]
    idx = np.empty(3 * n, np.uint32)
    idx[0::3], idx[1::3], idx[2::3] = u, s + np.uint32(num_private), i
    ptr = np.empty(3 * n + 1, np.int64)
    base = 3 * np.arange(n, dtype=np.int64)
    ptr[0:3 * n:3], ptr[1:3 * n:3], ptr[2:3 * n:3], ptr[3 * n] = base, base, base + 2, 3 * n
    return CSRData(r, ptr, idx, np.ones(3 * n, np.float32)), u, s, i

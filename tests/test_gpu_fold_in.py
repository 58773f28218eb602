"""Fold-in on the live model (svdf_fold_in, svdf_k_foldin.hip) on the GPU.  The reference is float64 numpy: A and b formed
in float64 from the float32 inputs, numpy.linalg.solve.  The yardstick of the accuracy bound is numpy's own float32 route on the same inputs."""
import numpy as np
import pytest

from test_gpu_rank_eval import new_trainer

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NU, NI, BASE = 300, 517, 3.0               # (base_score of cases.BASICMF_CONF)
LENGTHS = [0, 1, 15, 16, 17, 33, 300]      # stage edges, the second buffer, fewer ratings than k
F = 4                                       # the bound: e <= F * yardstick; the smallest power of two >= twice the largest measured ratio

_models = {}


def model(k):
    """a trainer of width k with a random normal item side and biases, and what was written, shared by the tests (write tests restore W_user)"""
    if k not in _models:
        rng = np.random.default_rng(k)
        t = new_trainer(NU, NI, k)
        m = dict(W_item=rng.standard_normal((NI, k)).astype(F32), i_bias=rng.standard_normal(NI).astype(F32), u_bias=rng.standard_normal(NU).astype(F32))
        for name, v in m.items():
            t.set_view(name, v)
        _models[k] = (t, m)
    return _models[k]


def sections(S, seed):
    """S sections of distinct users whose lengths cycle through LENGTHS from position S on, then one whose 20 items are each listed twice, then
    one that repeats the first user"""
    rng = np.random.default_rng(seed)
    users = rng.permutation(NU)[:S + 1].astype(np.uint32)
    items = [rng.integers(0, NI, LENGTHS[(S + s) % len(LENGTHS)]) for s in range(S)]
    items.append(np.tile(rng.permutation(NI)[:20], 2))
    items.append(rng.integers(0, NI, 9))
    users = np.append(users, users[0])
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in items])]).astype(np.int64)
    item = np.concatenate(items).astype(np.uint32)
    return users, ptr, item, rng.standard_normal(len(item)).astype(F32) + F32(BASE)


def solve(m, users, ptr, item, label, reg, dtype):
    """rows of the rule in `dtype`: Q^T Q + reg I and Q^T y formed and solved in it"""
    rows = np.zeros((len(users), m["W_item"].shape[1]), dtype)
    for s, u in enumerate(users):
        it = item[ptr[s]:ptr[s + 1]]
        if len(it):
            Q = m["W_item"][it].astype(dtype)
            y = label[ptr[s]:ptr[s + 1]].astype(dtype) - (dtype(BASE) + m["u_bias"][u].astype(dtype) + m["i_bias"][it].astype(dtype))
            rows[s] = np.linalg.solve(Q.T @ Q + dtype(reg) * np.eye(Q.shape[1], dtype=dtype), Q.T @ y)
    return rows


def worst(rows, want, ptr):
    live = np.diff(ptr) > 0
    return float((np.linalg.norm(rows[live].astype(F64) - want[live], axis=1) / np.linalg.norm(want[live], axis=1)).max())


@pytest.mark.parametrize("reg", [1.0, 2.0 ** -10])
@pytest.mark.parametrize("S", [1, 5, 203])
@pytest.mark.parametrize("k", [1, 3, 16, 17, 33, 64, 100, 128])
def test_rows_are_as_accurate_as_the_float32_route(k, S, reg):
    """block edges, a ragged last block and every width class; first, partial and many workgroups; well and poorly conditioned.
    Measured: the largest e / yardstick over the 48 cases is recorded in DESIGN.md 6an and profiles/r48_fold_in.md."""
    t, m = model(k)
    lists = sections(S, seed=1000 * k + S)
    before = t.counter(62)
    rows = t.fold_in(*lists, reg)
    assert rows.shape == (S + 2, k) and rows.dtype == F32 and t.counter(62) - before == S + 2
    want = solve(m, *lists, reg, F64)
    e, yard = worst(rows, want, lists[1]), max(worst(solve(m, *lists, reg, F32), want, lists[1]), 2.0 ** -20)
    print("fold_in k=%d S=%d reg=%g: e %.3e yardstick %.3e ratio %.3f" % (k, S, reg, e, yard, e / yard))
    assert e <= F * yard
    empty = np.diff(lists[1]) == 0
    assert not rows[empty].any() and not np.signbit(rows[empty]).any()


@pytest.mark.parametrize("k", [3, 64, 128])
def test_write_stores_the_rows_and_nothing_else(k):
    t, m = model(k)
    users, ptr, item, label = (x[:-1] if i == 0 else x for i, x in enumerate(sections(5, seed=k)))   # without the repeated user
    ptr = ptr[:-1]
    names = ("W_user", "u_bias", "W_item", "i_bias")
    before = {n: t.view(n) for n in names}
    kept = t.fold_in(users, ptr, item, label, 0.25, write=False)
    assert all(np.array_equal(t.view(n).view(np.uint32), before[n].view(np.uint32)) for n in names)
    rows = t.fold_in(users, ptr, item, label, 0.25, write=True)
    assert np.array_equal(rows.view(np.uint32), kept.view(np.uint32))
    after = {n: t.view(n) for n in names}
    assert np.array_equal(after["W_user"][users].view(np.uint32), rows.view(np.uint32))
    others = np.setdiff1d(np.arange(NU), users)
    assert np.array_equal(after["W_user"][others].view(np.uint32), before["W_user"][others].view(np.uint32))
    assert all(np.array_equal(after[n].view(np.uint32), before[n].view(np.uint32)) for n in names[1:])
    t.set_view("W_user", before["W_user"])


def test_a_folded_in_user_ranks_like_the_row_that_made_its_ratings():
    """a planted user at k = 16: 40 labels that are the float64 predictions of a hidden row; after fold_in(write=True) rank_topn lists what it
    lists with the hidden row written into W_user"""
    t, m = model(16)
    rng = np.random.default_rng(5)
    u, hidden = 7, rng.standard_normal(16).astype(F32)
    item = rng.permutation(NI)[:40].astype(np.uint32)
    W = m["W_item"].astype(F64)
    label = (BASE + F64(m["u_bias"][u]) + m["i_bias"][item].astype(F64) + W[item] @ hidden.astype(F64)).astype(F32)
    lists = (np.array([u], np.uint32), np.array([0, 40], np.int64), item, label)
    tops = []
    for row in (hidden.astype(F64), solve(m, *lists, 2.0 ** -20, F64)[0]):
        score = np.sort(m["i_bias"].astype(F64) + W @ row)[::-1]
        assert (score[:10] - score[1:11]).min() > 1e-3
        tops.append(np.argsort(-(m["i_bias"].astype(F64) + W @ row), kind="stable")[:10])
    assert np.array_equal(*tops)
    W_user = t.view("W_user")
    row = t.fold_in(*lists, 2.0 ** -20, write=True)[0]
    got = t.rank_topn(lists[0], 10)
    planted = W_user.copy()
    planted[u] = hidden
    t.set_view("W_user", planted)
    want = t.rank_topn(lists[0], 10)
    t.set_view("W_user", W_user)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0][0], tops[0]) and np.allclose(row, hidden, atol=1e-3)

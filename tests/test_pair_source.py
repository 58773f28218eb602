"""The rule that draws the negatives of a pass of rank pairs from a source of positives, without a GPU: the numpy
statement (tests/pair_source_rule.py), the library's host loop (svdf_pair_negatives), the stand-alone tool over the host-only header, and
every refusal on host-only handles -- before "needs a GPU"."""
import os
import subprocess

import numpy as np
import pytest

import cases
import pair_source_rule as rule
import rank_negs_rule
import svdfeature_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ([4, 4, 9], [10, 700, 10])


def host_trainer(fmt=0, extra=(), nu=20, ni=30):
    t = sa.Trainer(fmt, 3, 0, device=-2)
    for k, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=8) + list(extra):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


def source_rows(order, nu=300, ni=1200, n=4000, seed=11):
    """duplicate (user, item) rows, user 2 with one row, users 0 and 1 with none"""
    rng = np.random.default_rng(seed)
    u, p = rng.integers(3, nu, n), rng.integers(0, ni, n)
    u[0] = 2
    u[n // 2:n // 2 + 200], p[n // 2:n // 2 + 200] = u[:200], p[:200]
    if order == "grouped":
        at = np.argsort(u, kind="stable")
        u, p = u[at], p[at]
    return u.astype(np.uint32), p.astype(np.uint32)


def test_pinned_vectors():
    assert int(rule.stream(12345, 0)) == 0x6df61f806828913e and int(rule.stream(12345, 7)) == 0x0cee3333c9e3d7d8
    assert rule.draws(12345, 0, np.arange(6), 1200).tolist() == [607, 1083, 476, 1017, 945, 510]
    assert rule.draws(12345, 7, np.arange(8), 1200).tolist() == [496, 554, 32, 921, 199, 15, 1103, 184]
    for f in (lambda m, pos=PINNED[1]: rule.rule_negatives(10, 1200, PINNED[0], pos, m, 12345),
              lambda m, pos=PINNED[1]: sa.pair_negatives(10, 1200, PINNED[0], pos, m, 12345)):
        assert f(1).tolist() == [607, 549, 766]
        assert f(2).tolist() == [607, 549, 766, 1010, 64, 448]
        assert f(1, [10, 607, 10]).tolist()[0] == 1083   # 607 is the user's: the second draw


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_host_loop_is_the_numpy_rule(order):
    u, p = source_rows(order)
    uptr, items = rule.user_lists(300, u, p)
    for m in (1, 2, 5, 64):
        got = sa.pair_negatives(300, 1200, u, p, m, 2024)
        assert got.dtype == np.uint32 and np.array_equal(got, rule.rule_negatives(300, 1200, u, p, m, 2024))
        assert (got < 1200).all()
        owner = np.repeat(u, m).astype(np.int64)   # every negative outside P(user): no (user, negative) is a (user, positive) of the source
        assert not np.isin(owner * 1200 + got, u.astype(np.int64) * 1200 + p).any()
    assert uptr[1] == uptr[2] == 0 and uptr[3] - uptr[2] == 1


def test_seeds():
    u, p = source_rows("shuffled", n=500)
    a = sa.pair_negatives(300, 1200, u, p, 2, 5)
    assert np.array_equal(a, sa.pair_negatives(300, 1200, u, p, 2, 5))
    assert not np.array_equal(a, sa.pair_negatives(300, 1200, u, p, 2, 6))
    big = (1 << 63) + 5
    b = sa.pair_negatives(300, 1200, u, p, 2, big)
    assert not np.array_equal(a, b) and np.array_equal(b, rule.rule_negatives(300, 1200, u, p, 2, big))


def test_the_salt_separates_the_stream_from_rank_negatives():
    idx = np.arange(100)
    assert not (rule.stream(12345, idx) == rank_negs_rule.stream(12345, idx)).any()
    assert int(rule.stream(12345, 3)) == int(rank_negs_rule.stream(12345 ^ 0x70616972736E6567, 3))
    assert not np.array_equal(rule.draws(12345, idx, 0, 1200), rank_negs_rule.draws(12345, idx, 0, 1200))
    # the library's two functions on equal (seed, index): pair q of 100 one-row users with positive 0 against section q with positive 0, one
    # negative each -- both take the first draw of their stream that is not 0
    zero = np.zeros(100, np.uint32)
    pairs = sa.pair_negatives(100, 1200, idx, zero, 1, 12345).astype(np.int64)
    sections = lambda seed: sa.rank_negatives(1200, np.arange(101), zero, None, None, 1, seed)[:, 0].astype(np.int64)
    assert (pairs != sections(12345)).sum() >= 95   # (two independent ids of 1 199 agree with probability 1 / 1 199)
    assert np.array_equal(pairs, sections(12345 ^ 0x70616972736E6567))   # and the salt is what separates them


def test_density_limit():
    """6 300 of 6 400 items: every draw is accepted with probability exactly 1 / 64"""
    u, p = np.zeros(6300, np.uint32), np.arange(6300, dtype=np.uint32)
    full = sa.pair_negatives(1, 6400, u, p, 1, 7)
    assert (full >= 6300).all() and (full < 6400).all()
    want_full, took = rule.rule_negatives(1, 6400, u, p, 1, 7, return_draws=True)
    assert np.array_equal(full, want_full)
    # far below T: a pair needs more than T / 4 draws with probability (63 / 64)^1024 < 1e-7, one of 6 300 pairs with < 1e-3
    assert 64 < took.max() < rule.T / 4
    with pytest.raises(sa.SvdfError, match="pair_source: user 0 has 6301 distinct positive items of 6400.*svdf_dataset_from_pairs"):
        sa.pair_negatives(1, 6400, np.zeros(6301, np.uint32), np.arange(6301, dtype=np.uint32), 1, 7)
    # repeats do not count: 6 300 distinct items in 7 000 rows
    sa.pair_negatives(1, 6400, np.zeros(7000, np.uint32), np.concatenate([p, p[:700]]), 1, 7)


def test_uniformity():
    n = 90000
    neg = sa.pair_negatives(1, 100, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32) % 10, 1, 99)
    count = np.bincount(neg, minlength=100)
    assert count[:10].sum() == 0 and (np.abs(count[10:] - 1000) <= 150).all()


def test_refusals_on_the_host_function():
    for args, msg in (((20, 30, [], [], 1, 1), r"pair_source: a source needs at least one row \(n >= 1\)"),
                      ((20, 30, [1, 20], [2, 2], 1, 1), "user feature index exceed bound"),
                      ((20, 30, [1, 2], [2, 30], 1, 1), "item feature index exceed bound"),
                      ((20, 30, [1, 20], [30, 2], 1, 1), "item feature index exceed bound"),   # row by row
                      ((20, 30, [1, 2], [2, 3], 0, 1), "pair_source: num_neg must be between 1 and 256"),
                      ((20, 30, [1, 2], [2, 3], 257, 1), "pair_source: num_neg must be between 1 and 256"),
                      ((20, 30, [1, 2, 3], [2, 3], 1, 1), "pair_source: user and pos_item must have one entry per row")):
        with pytest.raises(sa.SvdfError, match=msg):
            sa.pair_negatives(*args)
    assert sa.pair_negatives(20, 30, [1, 2], [2, 3], 256, 1).shape == (512,)


def test_refusals_come_before_needs_a_gpu():
    t = host_trainer()
    for rows, msg in ((([], []), "pair_source: a source needs at least one row"), (([1, 20], [2, 2]), "user feature index exceed bound"),
                      (([1, 2], [2, 30]), "item feature index exceed bound"),
                      (([3] * 30, list(range(30))), "pair_source: user 3 has 30 distinct positive items of 30")):
        with pytest.raises(sa.SvdfError, match=msg):
            t.pair_source(*rows)
    with pytest.raises(sa.SvdfError, match="pair_source: call init_model / load_model and init_trainer first"):
        sa.Trainer(0, 3, 0, device=-2).pair_source([1], [2])
    src = t.pair_source([1, 2, 2], [2, 3, 3])   # a host-only handle's source: no device memory, every refusal of a pass
    other = host_trainer()
    for call in (lambda h, m: h.dataset_from_pair_source(src, m, 1), lambda h, m: h.pair_source_draw(src, m, 1)):
        for m in (0, 257, -1):
            with pytest.raises(sa.SvdfError, match="pair_source: num_neg must be between 1 and 256"):
                call(t, m)
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call(other, 1)
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call(t, 1)
    big = t.pair_source(np.ones(1 << 23, np.uint32), np.zeros(1 << 23, np.uint32))
    with pytest.raises(sa.SvdfError, match=r"pair_source: n \* num_neg must stay below 2\^31 - 16"):
        t.dataset_from_pair_source(big, 256, 1)
    big.close()
    # user-group trainers: what dataset_from_pairs says on the same handle
    g = host_trainer(fmt=1, extra=[("num_ufeedback", 30)])
    gs = g.pair_source([1], [2])
    for call in (lambda: g.dataset_from_pair_source(gs, 1, 1), lambda: g.dataset_from_pairs([1], [2], [3])):
        with pytest.raises(sa.SvdfError, match="dataset needs a GPU"):
            call()
    assert t.counter(44) == t.counter(45) == 0
    t.close()
    src.close()   # after its trainer
    src.close()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairsource_tool") / "check_pairsource_lists")
    subprocess.run(["c++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(ROOT, "svdfeature_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_pairsource_lists.cpp"), "-o", exe], check=True)
    return exe


def test_the_stand_alone_tool(tool):
    """built plain here; its header comment gives the sanitizer line for running it by hand"""
    out = subprocess.run([tool], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_the_tools_lists_and_negatives_are_numpys(tool, order):
    u, p = source_rows(order, nu=80, ni=150, n=700, seed=3)
    text = "80 150 700 3 %d\n" % ((1 << 63) + 9) + "".join("%d %d\n" % (a, b) for a, b in zip(u, p))
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    got = {line.split()[0]: np.array(line.split()[1:], np.int64) for line in out}
    uptr, items = rule.user_lists(80, u, p)
    assert np.array_equal(got["uptr"], uptr) and np.array_equal(got["uitems"], items)
    assert np.array_equal(got["neg"], rule.rule_negatives(80, 150, u, p, 3, (1 << 63) + 9))
    refused = subprocess.run([tool, "dump"], input="80 150 1 0 5\n1 1\n", capture_output=True, text=True, check=True).stdout
    assert refused.strip() == "refused pair_source: num_neg must be between 1 and 256"

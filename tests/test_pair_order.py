"""Shuffled passes of the pair source, without a GPU: the numpy statement of the order (tests/pair_order_rule.py), the
library's host loop (svdf_pair_order), the host twins on the permuted rows, the stand-alone tool over the host-only header, and every refusal
on host-only handles -- before "needs a GPU"."""
import os
import subprocess

import numpy as np
import pytest

import cases
import pair_hard_rule
import pair_order_rule as rule
import pair_source_rule
import pair_weight_rule
import svdfeature_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = (np.array([4, 4, 9], np.uint32), np.array([10, 700, 10], np.uint32))
SEEDS = (0, 12345, (1 << 63) + 5, (1 << 64) - 1)
SIZES = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 257, 4097, 100000)


def host_trainer(nu=20, ni=30):
    t = sa.Trainer(0, 3, 0, device=-2)
    for k, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=8):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


@pytest.fixture(scope="module")
def sigma_100k():
    return rule.sigma(100000, 12345)


def test_pinned_vectors():
    assert [int(k) for k in rule.keys(12345)] == [0x55f0c474c3817246, 0x212e2874c5b74625, 0x1b12a40bba019e32, 0xdbe2e77f7d83df15]
    for f in (rule.sigma, rule.sigma_scalar, sa.pair_order):
        assert f(10, 12345).tolist() == [2, 4, 8, 3, 7, 1, 6, 9, 0, 5]
        assert f(10, 12346).tolist() == [0, 8, 1, 6, 3, 9, 7, 5, 2, 4]
        assert f(1200, 12345)[:8].tolist() == [648, 161, 507, 552, 509, 792, 1082, 757]
        assert f(3, 12345).tolist() == [1, 2, 0] and f(2, 12345).tolist() == [1, 0] and f(1, 12345).tolist() == [0]
    assert rule.sigma(1, 12345, return_steps=True)[1].tolist() == [4]   # n = 1: after four applications
    # the pass of the pinned rows: the plain rule's negatives belong to positions, the rows come in the order 1, 2, 0
    s = sa.pair_order(3, 12345).astype(np.int64)
    u, p = PINNED[0][s], PINNED[1][s]
    for neg in (sa.pair_negatives(10, 1200, u, p, 1, 12345), pair_source_rule.rule_negatives(10, 1200, u, p, 1, 12345)):
        assert list(zip(u.tolist(), p.tolist(), neg.tolist())) == [(4, 700, 607), (9, 10, 549), (4, 10, 766)]


@pytest.mark.parametrize("n", SIZES)
def test_sigma_is_a_permutation_and_the_host_is_numpy(n):
    for seed in SEEDS:
        want = rule.sigma(n, seed)
        got = sa.pair_order(n, seed)
        assert got.dtype == np.uint32 and got.shape == (n,) and np.array_equal(got, want), seed
        assert np.array_equal(np.sort(want), np.arange(n)), seed
        if n <= 257:
            assert np.array_equal(want, rule.sigma_scalar(n, seed))


def test_two_order_seeds_give_two_orders():
    assert sa.pair_order(10, 12345).tolist() != sa.pair_order(10, 12346).tolist()
    assert len({tuple(sa.pair_order(10, s).tolist()) for s in range(20)}) >= 19
    assert np.array_equal(sa.pair_order(10, 12345 + (1 << 64)), sa.pair_order(10, 12345))   # order_seed is taken mod 2^64


def test_occupancy_of_the_first_tenth(sigma_100k):
    """the first 10 000 positions of 100 000 spread over ten equal ranges of source rows: each count within 15 % of 1000 -- 5 binomial standard
    deviations (sqrt(10000 * 0.1 * 0.9) = 30); the numpy statement stays within 7 %"""
    got = sa.pair_order(100000, 12345)
    assert np.array_equal(got, sigma_100k)
    count = np.bincount(got[:10000] // 10000, minlength=10)
    print("occupancy:", count.tolist())
    assert count.sum() == 10000 and (np.abs(count - 1000) <= 150).all()
    assert rule.sigma(100000, 12345, return_steps=True)[1].max() < 64   # far below the bound of 128


def test_a_grouped_source_comes_out_ungrouped():
    u, p = rule.grouped_rows()
    assert len(u) == 4000 and len(np.unique(u)) <= 300 and rule.same(u, np.arange(4000)) >= 3700
    for seed in SEEDS:
        after = rule.same(u, sa.pair_order(4000, seed))
        print("adjacent same-user rows after order_seed %d: %d" % (seed, after))
        assert 2 * after < 4000


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_host_twins_on_the_permuted_rows(order):
    """the shuffled rule is pair_negatives / pair_hard_negatives on (user[sigma], pos[sigma]): the negatives of the numpy rules on those rows,
    and -- P(u) and the tables do not depend on row order -- every negative outside its user's positives in the ORIGINAL rows"""
    u, p = pair_hard_rule.rows(order, n=700, seed=3)
    NU, NI = pair_hard_rule.NU, pair_hard_rule.NI
    s = sa.pair_order(len(u), 77).astype(np.int64)
    su, sp = u[s], p[s]
    held = u.astype(np.int64) * NI + p
    for m in (1, 3):
        neg = sa.pair_negatives(NU, NI, su, sp, m, 2024)
        assert np.array_equal(neg, pair_source_rule.rule_negatives(NU, NI, su, sp, m, 2024))
        assert not np.isin(np.repeat(su, m).astype(np.int64) * NI + neg, held).any()
        assert not np.array_equal(neg, sa.pair_negatives(NU, NI, u, p, m, 2024))   # the negatives belong to positions: another row order, another column
    w = pair_weight_rule.row_tables()["rows_300"]
    assert np.array_equal(sa.pair_negatives(NU, NI, su, sp, 2, 9, item_weight=w), pair_weight_rule.rule_negatives(NU, NI, su, sp, w, 2, 9))
    Wu, Wi, b = pair_hard_rule.model(16)
    got, score = sa.pair_hard_negatives(NU, NI, su, sp, 1, 4, 31, Wu, Wi, b, return_scores=True)
    want, want_score = pair_hard_rule.rule_hard(NU, NI, su, sp, 1, 4, 31, Wu, Wi, b)
    assert np.array_equal(got, want) and pair_hard_rule.same_scores(score, want_score)
    cand = pair_weight_rule.rule_negatives(NU, NI, su, sp, w, 4, 31).astype(np.int64).reshape(-1, 4)
    wwant, wscore, _ = pair_hard_rule.select(cand, pair_hard_rule.scores(cand, su, 1, Wu, Wi, b))
    wgot, wgot_score = sa.pair_hard_negatives(NU, NI, su, sp, 1, 4, 31, Wu, Wi, b, return_scores=True, item_weight=w)
    assert np.array_equal(wgot, wwant) and pair_hard_rule.same_scores(wgot_score, wscore)
    for f in (sa.pair_negatives, sa.pair_hard_negatives):
        assert "pair_order" in f.__doc__


def test_pair_order_refusals():
    for n in (0, -1):
        with pytest.raises(sa.SvdfError, match=r"pair_source: a source needs at least one row \(n >= 1\)"):
            sa.pair_order(n, 1)
    for n in ((1 << 31) - 16, 1 << 40):
        with pytest.raises(sa.SvdfError, match=r"pair_source: n \* num_neg must stay below 2\^31 - 16"):
            sa.pair_order(n, 1)


def test_refusals_come_before_needs_a_gpu():
    t, other = host_trainer(), host_trainer()
    ones = np.ones(30, np.uint32)
    for src in (t.pair_source([1, 2, 2], [2, 3, 3]), t.pair_source([1, 2, 2], [2, 3, 3], item_weight=ones)):
        for hard in (None, 1, 2):
            for call in (lambda h, m: h.dataset_from_pair_source(src, m, 1, hard=hard, shuffle=5), lambda h, m: h.pair_source_draw(src, m, 1, hard=hard, shuffle=5)):
                for m in (0, 257):
                    with pytest.raises(sa.SvdfError, match="pair_source: num_neg must be between 1 and 256"):
                        call(t, m)
                with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
                    call(other, 1)
                with pytest.raises(sa.SvdfError, match="needs a GPU"):
                    call(t, 1)
        for call in (lambda m, c: t.dataset_from_pair_source(src, m, 1, hard=c, shuffle=5), lambda m, c: t.pair_source_draw(src, m, 1, hard=c, shuffle=5)):
            for c in (0, -1, 257):
                with pytest.raises(sa.SvdfError, match="pair_source: num_cand must be between 1 and 256"):
                    call(1, c)
            with pytest.raises(sa.SvdfError, match="pair_source: num_neg \\* num_cand must be at most 256"):
                call(2, 200)
        with pytest.raises(sa.SvdfError, match="pair_source: return_scores needs hard="):
            t.pair_source_draw(src, 1, 1, return_scores=True, shuffle=5)
        src.close()
    assert [t.counter(c) for c in (44, 45, 46, 47, 48)] == [0, 0, 0, 0, 0]
    # the C entry points: num_cand = 0 is the plain pass (its refusals), a source that is NULL is "bad arguments", a rank handle's refusal is
    # the hard pass's
    import ctypes as C
    raw = C.CDLL(sa.load_library()._name)
    raw.svdf_dataset_from_pair_source_shuffled.restype = C.c_void_p
    raw.svdf_last_error.restype = C.c_char_p
    args = (C.c_void_p(t.h), None, 1, 0, C.c_uint64(1), C.c_uint64(2))
    assert raw.svdf_dataset_from_pair_source_shuffled(*args) is None and raw.svdf_last_error() == b"pair_source: bad arguments"
    buf = np.zeros(8, np.uint32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert raw.svdf_pair_source_draw_shuffled(*args, ptr, ptr, ptr, None) == -1 and raw.svdf_last_error() == b"pair_source: bad arguments"
    assert raw.svdf_pair_order(C.c_long(4), C.c_uint64(1), None) == -1 and raw.svdf_last_error() == b"pair_source: bad arguments"
    big = host_trainer(20, 30)
    n = 1 << 23
    src = big.pair_source(np.zeros(n, np.uint32), np.zeros(n, np.uint32))
    with pytest.raises(sa.SvdfError, match=r"pair_source: n \* num_neg must stay below 2\^31 - 16"):
        big.dataset_from_pair_source(src, 256, 1, shuffle=3)
    with pytest.raises(sa.SvdfError, match=r"pair_source: n \* num_neg \* num_cand must stay below 2\^31 - 16"):
        big.pair_source_draw(src, 1, 1, hard=256, shuffle=3)
    src.close()
    t.close()
    other.close()
    big.close()


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairorder_tool") / "check_pairorder_lists")
    subprocess.run(["c++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(ROOT, "svdfeature_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_pairorder_lists.cpp"), "-o", exe], check=True)
    return exe


def test_the_stand_alone_tool(tool):
    """built plain here; its header comment gives the sanitizer line for running it by hand"""
    out = subprocess.run([tool], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("n,seed", [(1, 0), (2, 12345), (65, (1 << 64) - 1), (1025, 12345), (4097, (1 << 63) + 5)])
def test_the_tools_order_is_numpys(tool, n, seed):
    out = subprocess.run([tool, "dump"], input="%d %d 128\n" % (n, seed), capture_output=True, text=True, check=True).stdout.splitlines()
    got = {line.split()[0]: np.array(line.split()[1:], np.int64) for line in out}
    want, steps = rule.sigma(n, seed, return_steps=True)
    assert np.array_equal(got["sigma"], want) and np.array_equal(got["steps"], steps)


def test_the_tools_exhaustion_with_two_steps(tool):
    """the bound lowered to 2 applications: the first position that needs a third is named, in the published words"""
    n, seed = 1025, 12345
    steps = rule.sigma(n, seed, return_steps=True)[1]
    first = int(np.flatnonzero(steps > 2)[0])
    out = subprocess.run([tool, "dump"], input="%d %d 2\n" % (n, seed), capture_output=True, text=True, check=True).stdout
    assert out.strip() == "refused pair_source: order_seed 12345 needs more than 2 steps at position %d; take another order_seed" % first
    with pytest.raises(AssertionError, match="needs more than 2 steps at position %d" % first):
        rule.sigma(n, seed, walks=2)
    for text, msg in (("0 1 128\n", "pair_source: a source needs at least one row (n >= 1)"), ("2147483632 1 128\n", "pair_source: n * num_neg must stay below 2^31 - 16")):
        assert subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout.strip() == "refused " + msg

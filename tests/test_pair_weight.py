"""Item-weighted negatives for the pair source, without a GPU: the numpy / Python-integer statement of the rule
(tests/pair_weight_rule.py), the library's host loops (svdf_pair_negatives_weighted, svdf_pair_hard_negatives_weighted), the map in both
forms on every boundary word of its tables (svdf_pair_weight_lookup on the host), the stand-alone tool over the host-only header, and every
refusal on host-only handles -- before "needs a GPU"."""
import os
import subprocess

import numpy as np
import pytest

import cases
import pair_hard_rule
import pair_source_rule
import pair_weight_rule as rule
import svdfeature_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ([4, 4, 9], [10, 700, 10])
FULL = (1 << 32) - 1
TABLES = rule.tables()


def host_trainer(nu=20, ni=30):
    t = sa.Trainer(0, 3, 0, device=-2)
    for k, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=8):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


def test_pinned_vectors():
    w = rule.pinned_weights()
    cdf = rule.cdf_of(w)
    assert cdf[-1] == 50185
    assert rule.wdraws(12345, 0, np.arange(6), cdf).tolist() == [611, 1086, 472, 1016, 936, 514]
    assert rule.wdraws(12345, 7, np.arange(8), cdf).tolist() == [502, 551, 33, 918, 200, 19, 1102, 177]
    for form in (1, 2):
        assert sa.pair_weight_lookup(w, rule.words(12345, 0, np.arange(6)), form).tolist() == [611, 1086, 472, 1016, 936, 514]
        assert sa.pair_weight_lookup(w, rule.words(12345, 7, np.arange(8)), form).tolist() == [502, 551, 33, 918, 200, 19, 1102, 177]
    for f in (lambda m: rule.rule_negatives(10, 1200, PINNED[0], PINNED[1], w, m, 12345),
              lambda m: sa.pair_negatives(10, 1200, PINNED[0], PINNED[1], m, 12345, item_weight=w)):
        assert f(1).tolist() == [611, 547, 755]
        assert f(2).tolist() == [611, 547, 755, 1006, 59, 447]
    assert ((((1 << 64) - 1) * FULL) >> 64) == FULL - 1 == 4294967294
    top = np.zeros(3, np.uint32)
    top[0], top[2] = FULL - 1, 1   # W = 2^32 - 1: the last word gives y = W - 1, the one unit of item 2; one word earlier still does
    assert sa.pair_weight_lookup(top, np.array([(1 << 64) - 1, (1 << 64) - (1 << 32) - 1, (1 << 64) - (1 << 32) - 2], np.uint64)).tolist() == [2, 2, 0]


def test_equal_weights_are_not_the_uniform_source():
    """the uniform map uses the high 32 bits of the word, this one all 64: the two agree on all but about num_item of every 2^32 words, so
    nothing promises equal negatives.  A word on which they differ: high half h with h * 300 = 2^32 - 4 (mod 2^32), low half all ones."""
    ones = np.ones(rule.NI, np.uint32)
    h = ((1 << 30) - 1) * pow(75, -1, 1 << 30) % (1 << 30)
    assert (h * 300) % (1 << 32) == (1 << 32) - 4
    x = (h << 32) | 0xFFFFFFFF
    uniform = ((x >> 32) * 300) >> 32
    assert rule.lookup(rule.cdf_of(ones), x) == uniform + 1
    for form in (1, 2):
        assert sa.pair_weight_lookup(ones, [x, x - 0xFFFFFFFF], form).tolist() == [uniform + 1, uniform]
    u, p = rule.rows("shuffled", n=500)
    equal = sa.pair_negatives(rule.NU, rule.NI, u, p, 1, 3, item_weight=ones)
    assert np.array_equal(equal, rule.rule_negatives(rule.NU, rule.NI, u, p, ones, 1, 3))


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_host_loop_is_the_numpy_rule(order):
    u, p = rule.rows(order)
    for name, w in rule.row_tables().items():
        for m in (1, 2, 7, 256):
            got = sa.pair_negatives(rule.NU, rule.NI, u, p, m, 2024, item_weight=w)
            assert got.dtype == np.uint32 and np.array_equal(got, rule.rule_negatives(rule.NU, rule.NI, u, p, w, m, 2024)), (name, m)
            assert (w[got] > 0).all()   # no zero-weight item is ever drawn
            owner = np.repeat(u, m).astype(np.int64)
            assert not np.isin(owner * rule.NI + got, u.astype(np.int64) * rule.NI + p).any()


@pytest.mark.parametrize("m,C", [(1, 2), (1, 8), (3, 4), (1, 65)])
def test_hard_host_rule_is_numpys(m, C):
    u, p = rule.rows("shuffled", n=600)
    w = rule.row_tables()["rows_300"]
    cand = rule.rule_negatives(rule.NU, rule.NI, u, p, w, m * C, 31).astype(np.int64).reshape(-1, C)
    for k in (1, 5, 16, 64):
        Wu, Wi, b = pair_hard_rule.model(k)
        sc = pair_hard_rule.scores(cand, u, m, Wu, Wi, b)
        want, want_score, untied = pair_hard_rule.select(cand, sc)
        got, got_score = sa.pair_hard_negatives(rule.NU, rule.NI, u, p, m, C, 31, Wu, Wi, b, return_scores=True, item_weight=w)
        assert np.array_equal(got, want) and pair_hard_rule.same_scores(got_score, want_score), (k, int((got != want).sum()))
    # hard = 1 is the weighted plain pass
    Wu, Wi, b = pair_hard_rule.model(5)
    assert np.array_equal(sa.pair_hard_negatives(rule.NU, rule.NI, u, p, m, 1, 31, Wu, Wi, b, item_weight=w),
                          sa.pair_negatives(rule.NU, rule.NI, u, p, m, 31, item_weight=w))


@pytest.mark.parametrize("name", sorted(TABLES))
def test_lookup_on_every_boundary_word(name):
    w = TABLES[name]
    cdf = rule.cdf_of(w)
    x = rule.boundary_words(cdf)
    want = rule.lookups(cdf, x, exact=True)
    assert (w[want] > 0).all() and np.array_equal(want, rule.lookups(cdf, x))
    assert all(rule.lookup(cdf, int(v)) == i for v, i in zip(x[:50].tolist(), want[:50].tolist()))   # ... and bisect itself
    assert want[0] == np.flatnonzero(w)[0] and want[-1] == np.flatnonzero(w)[-1]   # x = 0 and x = 2^64 - 1
    for form in (1, 2):
        assert np.array_equal(sa.pair_weight_lookup(w, x, form), want), form
    # the words between the boundaries: each positive item's first word x0 and its x0 - 1 map to the item and to the positive item before it
    positive = np.flatnonzero(w)
    first = np.array([-((-cdf[i] << 64) // cdf[-1]) for i in positive.tolist()], dtype=np.uint64)
    assert np.array_equal(sa.pair_weight_lookup(w, first, 2), positive)
    if len(positive) > 1:
        assert np.array_equal(sa.pair_weight_lookup(w, first[1:] - np.uint64(1), 2), positive[:-1])


def test_guide_table_of_the_tool_is_the_published_one(tool):
    w = TABLES["zero_across_edge"]
    text = "3 %d 2 1 5 2\n" % len(w) + " ".join(str(v) for v in w.tolist()) + "\n1 0\n2 5\n"
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in out}
    cdf = rule.cdf_of(w)
    assert got["cdf"] == cdf and got["guide"] == rule.guide_of(cdf)[1] and len(got["guide"]) == 257


def test_class_frequencies():
    """5 000 pairs x 40 draws under the pinned weights, items classed by id % 8: every class count lies within 5 binomial standard deviations
    of draws * W_class / W (the map's bias, W / 2^64 per draw, is far below one count).  The bound is derived, not tuned; the numpy statement
    gives 1.934 deviations at worst (class 3)."""
    w = rule.pinned_weights()
    cdf = rule.cdf_of(w)
    x = rule.words(777, np.arange(5000)[:, None], np.arange(40)[None, :]).ravel()
    ids = sa.pair_weight_lookup(w, x, 2)
    assert np.array_equal(ids, rule.lookups(cdf, x)) and np.array_equal(ids, sa.pair_weight_lookup(w, x, 1))
    draws, W = len(x), cdf[-1]
    worst = 0.0
    for c in range(8):
        prob = int(w[c::8].astype(np.int64).sum()) / W
        dev = abs(int((ids % 8 == c).sum()) - draws * prob) / np.sqrt(draws * prob * (1 - prob))
        worst = max(worst, dev)
        assert dev <= 5.0, (c, dev)
    print("class frequencies: worst deviation %.2f sigma" % worst)


def test_weighted_density_rule():
    # 128 items: the user of items 0 .. 126 holds 6 300 of W = 6 400 -- 64 * (W - held) == W, accepted; every negative is item 127
    w = np.ones(128, np.uint32)
    w[0], w[127] = 6300 - 126, 100
    u, p = np.zeros(127, np.uint32), np.arange(127, dtype=np.uint32)
    assert rule.density_refusal(2, u, p, w) is None
    neg = sa.pair_negatives(2, 128, u, p, 4, 7, item_weight=w)
    assert (neg == 127).all()
    # the COUNT rule refuses those rows (127 of 128 items): a weighted source applies the weighted rule in its place
    with pytest.raises(sa.SvdfError, match="pair_source: user 0 has 127 distinct positive items of 128"):
        sa.pair_negatives(2, 128, u, p, 4, 7)
    w[127] = 99   # one unit less
    assert rule.density_refusal(2, u, p, w) == (0, 6300, 6399)
    with pytest.raises(sa.SvdfError, match="pair_source: user 0's positive items hold 6300 of the total item weight 6399: less than 1 part in 64 is left "
                                           r"to draw a negative from; draw its negatives yourself \(svdf_dataset_from_pairs\)"):
        sa.pair_negatives(2, 128, u, p, 4, 7, item_weight=w)
    # a user whose two popular positives hold more than 63 / 64 of W is refused; the unweighted rule admits it; the first such user is named
    pop = np.ones(1000, np.uint32)
    pop[[3, 8]] = 40000
    uu, pp = np.array([5, 2, 2, 7], np.uint32), np.array([3, 3, 8, 8], np.uint32)
    assert rule.density_refusal(10, uu, pp, pop) == (2, 80000, 80998)
    with pytest.raises(sa.SvdfError, match="pair_source: user 2's positive items hold 80000 of the total item weight 80998"):
        sa.pair_negatives(10, 1000, uu, pp, 1, 7, item_weight=pop)
    assert sa.pair_negatives(10, 1000, uu, pp, 1, 7).shape == (4,)
    t = host_trainer(10, 1000)
    with pytest.raises(sa.SvdfError, match="pair_source: user 2's positive items hold 80000 of the total item weight 80998"):
        t.pair_source(uu, pp, item_weight=pop)
    t.pair_source(uu, pp).close()
    t.close()


def test_sum_refusals():
    zero, big = np.zeros(30, np.uint32), np.zeros(30, np.uint32)
    big[3], big[29] = FULL, 1
    for call in (lambda w: sa.pair_negatives(20, 30, [1, 2], [2, 3], 1, 1, item_weight=w),
                 lambda w: sa.pair_hard_negatives(20, 30, [1, 2], [2, 3], 1, 2, 1, np.zeros((20, 4), np.float32), np.zeros((30, 4), np.float32),
                                                  np.zeros(30, np.float32), item_weight=w),
                 lambda w: sa.pair_weight_lookup(w, [0, 1], 1)):
        with pytest.raises(sa.SvdfError, match="pair_source: the item weights sum to 0$"):
            call(zero)
        with pytest.raises(sa.SvdfError, match=r"pair_source: the item weights sum to 4294967296: the sum must stay below 2\^32"):
            call(big)
    big[29] = 0   # 2^32 - 1 is the largest sum
    assert sa.pair_negatives(20, 30, [1, 2], [2, 4], 1, 1, item_weight=big).tolist() == [3, 3]
    # the rows and the pass come first, as in the unweighted call
    for args, msg in (((20, 30, [1, 20], [2, 2], 1, 1), "user feature index exceed bound"), ((20, 30, [1, 2], [2, 30], 1, 1), "item feature index exceed bound"),
                      ((20, 30, [1, 2], [2, 3], 0, 1), "pair_source: num_neg must be between 1 and 256"), ((20, 30, [], [], 1, 1), "pair_source: a source needs at least one row")):
        with pytest.raises(sa.SvdfError, match=msg):
            sa.pair_negatives(*args, item_weight=zero)
    for bad in (np.ones(29, np.uint32), np.ones(31, np.uint32), np.ones((2, 15), np.uint32)):
        with pytest.raises(sa.SvdfError, match="pair_source: item_weight must have one entry per item"):
            sa.pair_negatives(20, 30, [1, 2], [2, 3], 1, 1, item_weight=bad)
    for bad in (np.full(30, -1), np.full(30, 1 << 32), np.ones(30, np.float64)):
        with pytest.raises(sa.SvdfError, match="pair_source: item_weight must hold integers"):
            sa.pair_negatives(20, 30, [1, 2], [2, 3], 1, 1, item_weight=bad)
    with pytest.raises(sa.SvdfError, match="pair_weight_lookup: bad arguments"):
        sa.pair_weight_lookup(np.ones(30, np.uint32), [0], 3)


def test_refusals_come_before_needs_a_gpu():
    t = host_trainer()
    ones, zero, big = np.ones(30, np.uint32), np.zeros(30, np.uint32), np.zeros(30, np.uint32)
    big[[0, 1]] = 1 << 31
    heavy = ones.copy()
    heavy[5] = 10000
    for rows, w, msg in ((([], []), ones, "pair_source: a source needs at least one row"), (([1, 20], [2, 2]), zero, "user feature index exceed bound"),
                         (([1, 2], [2, 30]), zero, "item feature index exceed bound"), (([1, 2], [2, 3]), zero, "pair_source: the item weights sum to 0"),
                         (([1, 2], [2, 3]), big, r"pair_source: the item weights sum to 4294967296: the sum must stay below 2\^32"),
                         (([1, 2], [2, 3]), ones[:29], "pair_source: item_weight must have one entry per item"),
                         (([1, 3, 3], [2, 5, 6]), heavy, "pair_source: user 3's positive items hold 10001 of the total item weight 10029")):
        with pytest.raises(sa.SvdfError, match=msg):
            t.pair_source(*rows, item_weight=w)
    with pytest.raises(sa.SvdfError, match="pair_source: call init_model / load_model and init_trainer first"):
        sa.Trainer(0, 3, 0, device=-2).pair_source([1], [2], item_weight=ones)
    src = t.pair_source([1, 2, 2], [2, 3, 3], item_weight=heavy)   # a host-only handle's weighted source: no device memory, every refusal of a pass
    other = host_trainer()
    for call in (lambda h, m: h.dataset_from_pair_source(src, m, 1), lambda h, m: h.pair_source_draw(src, m, 1),
                 lambda h, m: h.dataset_from_pair_source(src, m, 1, hard=2), lambda h, m: h.pair_source_draw(src, m, 1, hard=2)):
        for m in (0, 257):
            with pytest.raises(sa.SvdfError, match="pair_source: num_neg must be between 1 and 256"):
                call(t, m)
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call(other, 1)
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call(t, 1)
    with pytest.raises(sa.SvdfError, match="pair_source: num_neg \\* num_cand must be at most 256"):
        t.pair_source_draw(src, 2, 1, hard=200)
    with pytest.raises(sa.SvdfError, match="pair_source: the item weights sum to 0"):   # the probe validates before it needs the device
        sa.pair_weight_lookup(zero, [0], 1, trainer=t)
    with pytest.raises(sa.SvdfError, match="needs a GPU"):
        sa.pair_weight_lookup(ones, [0], 1, trainer=t)
    assert t.counter(44) == t.counter(45) == t.counter(46) == t.counter(47) == 0
    t.set_knob("pair_weight_form", 2)
    with pytest.raises(sa.SvdfError):
        t.set_knob("pair_weight_form", 3)
    t.close()
    src.close()   # after its trainer
    src.close()


def test_none_is_the_old_call():
    u, p = rule.rows("shuffled", n=700)
    Wu, Wi, b = pair_hard_rule.model(16)
    for m in (1, 3):
        old = pair_source_rule.rule_negatives(rule.NU, rule.NI, u, p, m, 9)
        assert np.array_equal(sa.pair_negatives(rule.NU, rule.NI, u, p, m, 9), old)
        assert np.array_equal(sa.pair_negatives(rule.NU, rule.NI, u, p, m, 9, item_weight=None), old)
        a = sa.pair_hard_negatives(rule.NU, rule.NI, u, p, m, 4, 9, Wu, Wi, b, return_scores=True)
        c = sa.pair_hard_negatives(rule.NU, rule.NI, u, p, m, 4, 9, Wu, Wi, b, return_scores=True, item_weight=None)
        want = pair_hard_rule.rule_hard(rule.NU, rule.NI, u, p, m, 4, 9, Wu, Wi, b)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[0], want[0]) and np.array_equal(a[1].view(np.uint32), c[1].view(np.uint32))
    # the C entry point with a NULL table is the unweighted one (a second handle on the library: its own argument types)
    import ctypes as C
    raw = C.CDLL(sa.load_library()._name)
    neg = np.zeros(700, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert raw.svdf_pair_negatives_weighted(C.c_long(rule.NU), C.c_long(rule.NI), C.c_long(700), ptr(u), ptr(p), None, 1, C.c_uint64(9), ptr(neg)) == 0
    assert np.array_equal(neg, pair_source_rule.rule_negatives(rule.NU, rule.NI, u, p, 1, 9))


def test_popularity_weights():
    pos = np.array([3] * 4 + [7] * 2 + [0] + [9] * 16, np.int64)
    w = sa.pair_popularity_weights(pos, 12)
    assert w.dtype == np.uint32 and w.tolist() == [1024, 1, 1, int(np.rint(1024 * 4 ** 0.75)), 1, 1, 1, int(np.rint(1024 * 2 ** 0.75)), 1, 8192, 1, 1]
    assert sa.pair_popularity_weights(pos, 12, power=1.0, unseen=0).tolist() == [1024, 0, 0, 4096, 0, 0, 0, 2048, 0, 16384, 0, 0]
    with pytest.raises(sa.SvdfError, match="the item weights sum to .*: the sum must stay below 2\\^32"):
        sa.pair_popularity_weights(np.zeros(1 << 23, np.int64), 2, power=1.0)
    with pytest.raises(sa.SvdfError, match="item feature index exceed bound"):
        sa.pair_popularity_weights(pos, 9)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairweight_tool") / "check_pairweight_lists")
    subprocess.run(["c++", "-std=c++17", "-O1", "-pthread", "-I" + os.path.join(ROOT, "svdfeature_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_pairweight_lists.cpp"), "-o", exe], check=True)
    return exe


def test_the_stand_alone_tool(tool):
    """built plain here; its header comment gives the sanitizer line for running it by hand"""
    out = subprocess.run([tool], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("order,form", [("grouped", 1), ("shuffled", 2)])
def test_the_tools_tables_and_negatives_are_numpys(tool, order, form):
    u, p = rule.rows(order, n=700, seed=3)
    w = rule.row_tables()["rows_300"]
    seed = (1 << 63) + 9
    text = "%d %d 700 3 %d %d\n" % (rule.NU, rule.NI, seed, form) + " ".join(str(v) for v in w.tolist()) + "\n" + "".join("%d %d\n" % (a, b) for a, b in zip(u, p))
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    got = {line.split()[0]: np.array(line.split()[1:], np.int64) for line in out}
    cdf = rule.cdf_of(w)
    assert got["cdf"].tolist() == cdf and got["guide"].tolist() == rule.guide_of(cdf)[1]
    assert np.array_equal(got["neg"], rule.rule_negatives(rule.NU, rule.NI, u, p, w, 3, seed))
    refused = subprocess.run([tool, "dump"], input="3 4 1 1 5 1\n0 0 0 0\n1 1\n", capture_output=True, text=True, check=True).stdout
    assert refused.strip() == "refused pair_source: the item weights sum to 0"

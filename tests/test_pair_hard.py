"""Hard negatives for passes of a pair source (svdf_pair_hard_negatives / svdf_*_pair_source*_hard), without a GPU: the
numpy statement of the rule (tests/pair_hard_rule.py) against the library's host loop and the stand-alone tool over the host-only header,
ties, +-0, NaN and +-inf scores, inputs on which a wrong summation order changes the chosen negatives, and every refusal on host-only
handles -- before "needs a GPU"."""
import os
import subprocess

import numpy as np
import pytest

import cases
import pair_hard_rule as hard
import rank_rounding
from pair_hard_rule import N, NI, NU, SHAPES, inf_model, model, nan_model, rounding_model, rows, tie_model, zero_model
import svdfeature_amd as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
WIDTHS = (1, 3, 4, 5, 7, 16, 64)
PINNED = ([4, 4, 9], [10, 700, 10])


def check(u, p, m, C, seed, W):
    """the library's host loop against the numpy rule: ids, and scores bit for bit; returns the rule's full answer"""
    want = hard.rule_hard(NU, NI, u, p, m, C, seed, *W, full=True)
    neg, score = sa.pair_hard_negatives(NU, NI, u, p, m, C, seed, *W, return_scores=True)
    assert neg.dtype == np.uint32 and neg.shape == (len(u) * m,) and np.array_equal(neg, want[0])
    assert hard.same_scores(score, want[1])
    assert np.array_equal(sa.pair_hard_negatives(NU, NI, u, p, m, C, seed, *W), neg)
    return want


def test_pinned_vectors():
    cand = hard.candidates(10, 1200, *PINNED, 1, 2, 12345)
    assert cand.tolist() == [[607, 549], [766, 1010], [64, 448]]
    assert cand.ravel().tolist() == sa.pair_negatives(10, 1200, *PINNED, 2, 12345).tolist()
    zero, up = np.zeros((10, 4), F32), np.arange(1200, dtype=F32)
    for f in (lambda b: hard.rule_hard(10, 1200, *PINNED, 1, 2, 12345, zero, np.zeros((1200, 4), F32), b),
              lambda b: sa.pair_hard_negatives(10, 1200, *PINNED, 1, 2, 12345, zero, np.zeros((1200, 4), F32), b, return_scores=True)):
        neg, score = f(up)
        assert neg.tolist() == [607, 1010, 448] and score.tolist() == [607.0, 1010.0, 448.0]
        neg, score = f(-up)
        assert neg.tolist() == [549, 766, 64] and score.tolist() == [-549.0, -766.0, -64.0]


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("m,C", SHAPES)
def test_host_loop_is_the_numpy_rule(order, m, C):
    u, p = rows(order)
    picked = 0
    for k in WIDTHS:
        neg, _, cand, sc, untied = check(u, p, m, C, 2024 + k, model(k))
        owner = np.repeat(u, m).astype(np.int64)   # every negative outside P(user)
        assert not np.isin(owner * NI + neg, u.astype(np.int64) * NI + p).any()
        assert np.array_equal(sc[np.arange(len(neg)), (cand == neg[:, None]).argmax(1)].view(np.uint32), sc.max(1).view(np.uint32))
        picked += int((neg != cand[:, 0]).sum())
    assert C == 1 or picked > len(WIDTHS) * N * m // 4   # the choice is not the first candidate


def test_one_candidate_is_the_plain_pass():
    u, p = rows("shuffled")
    for m in (1, 3, 256):
        plain = sa.pair_negatives(NU, NI, u[:500], p[:500], m, 9)
        assert np.array_equal(sa.pair_hard_negatives(NU, NI, u[:500], p[:500], m, 1, 9, *model(5)), plain)
        assert np.array_equal(hard.rule_hard(NU, NI, u[:500], p[:500], m, 1, 9, *model(5))[0], plain)


def test_equal_scores_go_to_the_smaller_id():
    u, p = rows("shuffled")
    neg, _, cand, sc, untied = check(u, p, 1, 8, 3, tie_model())
    twin = (cand % (NI // 2) == (neg % (NI // 2))[:, None]) & (cand != neg[:, None])   # the chosen row's other id among the candidates
    assert twin.any(1).sum() > 30 and (~untied).sum() > 30
    assert (neg[twin.any(1)] < NI // 2).all()
    neg, score, cand, _, untied = check(u, p, 2, 8, 4, zero_model())
    assert np.array_equal(neg, cand.min(1)) and (neg != cand[:, 0]).sum() > 1000
    assert (score == 0).all()


def test_nan_and_inf_scores():
    u, p = rows("shuffled")
    u[10:40] = 5
    u[40:60] = 7
    for C in (4, 70):
        neg, score, cand, sc, _ = check(u, p, 1, C, 5, nan_model())
        lost = np.isin(u, (5, 7))
        assert np.array_equal(neg[lost], cand[lost, 0]) and np.isnan(score[lost]).all() and np.isnan(sc[lost]).all()
        some = ~np.isnan(sc).all(1)
        assert not some[lost].any() and (C == 4 or some[~lost].all())   # (with 4 candidates a pair may draw four NaN items)
        assert not np.isnan(score[some]).any() and (neg[some] % 3 != 0).all()
        assert np.array_equal(neg[~some], cand[~some, 0])
    neg, score, cand, sc, _ = check(u, p, 1, 8, 6, inf_model())
    has = np.isposinf(sc).any(1)
    assert has.sum() > 500 and np.isposinf(score[has]).all() and (neg[has] % 10 == 5).all()
    only_minus = np.isneginf(sc).all(1)
    assert np.array_equal(neg[only_minus], cand[only_minus].min(1))
    assert (np.isneginf(score) == only_minus).all()


# ---- inputs on which a wrong summation order changes the chosen negatives.  The bound is a CONDITION on the inputs, checked here on the
# CPU: at least 20 of the 3 000 chosen negatives move under every decoy order that is a different computation at the width.
ROUNDING_WIDTHS = (5, 7, 16, 64, 128, 256)


def rounding_decoys(k):
    """"eight" equals the pinned order up to two chunks"""
    return [d for d in rank_rounding.DOT_DECOYS if d != "eight" or k >= 12]


@pytest.mark.parametrize("k", ROUNDING_WIDTHS)
def test_the_rounding_inputs_tell_wrong_orders_apart(k):
    u, p = rows("shuffled")
    W = rounding_model(k)
    neg = check(u, p, 1, 8, 11, W)[0]
    for decoy in rounding_decoys(k):
        moved = int((hard.rule_hard(NU, NI, u, p, 1, 8, 11, *W, order=decoy)[0] != neg).sum())
        assert moved >= 20, (k, decoy, moved)


# ---- refusals, reached on host-only handles
def host_trainer(fmt=0, extra=(), nu=20, ni=30):
    t = sa.Trainer(fmt, 3, 0, device=-2)
    for k, v in cases.conf_with(cases.PAIR_CONF, num_user=nu, num_item=ni, num_factor=8) + list(extra):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


BOUNDS = [((0, 2), "pair_source: num_neg must be between 1 and 256"), ((257, 1), "pair_source: num_neg must be between 1 and 256"),
          ((1, 0), "pair_source: num_cand must be between 1 and 256"), ((1, 257), "pair_source: num_cand must be between 1 and 256"),
          ((1, -1), "pair_source: num_cand must be between 1 and 256"), ((2, 129), "pair_source: num_neg \\* num_cand must be at most 256"),
          ((256, 256), "pair_source: num_neg \\* num_cand must be at most 256")]


def test_refusals_come_before_needs_a_gpu(tmp_path):
    t, other = host_trainer(), host_trainer()
    src = t.pair_source([1, 2, 2], [2, 3, 3])
    calls = (lambda h, s, m, C: h.dataset_from_pair_source(s, m, 1, hard=C), lambda h, s, m, C: h.pair_source_draw(s, m, 1, hard=C),
             lambda h, s, m, C: h.pair_source_draw(s, m, 1, hard=C, return_scores=True))
    for call in calls:
        for (m, C), msg in BOUNDS:
            with pytest.raises(sa.SvdfError, match=msg):
                call(t, src, m, C)
        with pytest.raises(sa.SvdfError, match="pair_source: the source was created on another trainer"):
            call(other, src, 1, 2)
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call(t, src, 1, 2)
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call(t, src, 4, 64)
    big = t.pair_source(np.ones(1 << 23, np.uint32), np.zeros(1 << 23, np.uint32))
    for call in calls:
        with pytest.raises(sa.SvdfError, match=r"pair_source: n \* num_neg \* num_cand must stay below 2\^31 - 16"):
            call(t, big, 16, 16)
    big.close()
    with pytest.raises(sa.SvdfError, match="pair_source: return_scores needs hard="):
        t.pair_source_draw(src, 1, 1, return_scores=True)
    # the trainers svdf_rank_topn does not admit, in its words
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    for h, msg in ((host_trainer(fmt=1, extra=[("num_ufeedback", 30)]), "pair_source: user-group trainers .*are not covered"),
                   (host_trainer(extra=[("feature_item", str(table))]), "pair_source: feature_user / feature_item side tables change the score"),
                   (host_trainer(extra=[("feature_user", str(table))]), "pair_source: feature_user / feature_item side tables change the score"),
                   (host_trainer(extra=[("amd:gpus", 2)]), "pair_source: amd:gpus > 1 is not covered")):
        hs = h.pair_source([1], [2])
        for call in calls:
            with pytest.raises(sa.SvdfError, match=msg):
                call(h, hs, 1, 2)
            with pytest.raises(sa.SvdfError, match="pair_source: num_cand must be between 1 and 256"):   # the bounds first
                call(h, hs, 1, 0)
    assert t.counter(44) == t.counter(45) == t.counter(46) == 0
    t.set_knob("pair_hard_form", 2)
    with pytest.raises(sa.SvdfError, match="pair_hard_form must be 0"):
        t.set_knob("pair_hard_form", 3)
    t.close()
    src.close()


def test_refusals_on_the_host_function():
    W = (np.zeros((20, 4), F32), np.zeros((30, 4), F32), np.zeros(30, F32))
    for (m, C), msg in BOUNDS:
        with pytest.raises(sa.SvdfError, match=msg):
            sa.pair_hard_negatives(20, 30, [1, 2], [2, 3], m, C, 1, *W)
    for args, msg in ((([], [], 1, 2), r"pair_source: a source needs at least one row \(n >= 1\)"),
                      (([1, 20], [2, 2], 1, 2), "user feature index exceed bound"), (([1, 2], [2, 30], 1, 2), "item feature index exceed bound"),
                      (([1, 2, 3], [2, 3], 1, 2), "pair_source: user and pos_item must have one entry per row")):
        with pytest.raises(sa.SvdfError, match=msg):
            sa.pair_hard_negatives(20, 30, *args, 1, *W)
    with pytest.raises(sa.SvdfError, match="pair_source: W_user, W_item and i_bias must be"):
        sa.pair_hard_negatives(20, 30, [1], [2], 1, 2, 1, W[0], W[1][:29], W[2])
    with pytest.raises(sa.SvdfError, match="pair_source: hard negatives need num_factor between 1 and 1024"):
        sa.pair_hard_negatives(20, 30, [1], [2], 1, 2, 1, np.zeros((20, 1025), F32), np.zeros((30, 1025), F32), W[2])
    assert sa.pair_hard_negatives(20, 30, [1, 2], [2, 3], 4, 64, 1, *W).shape == (8,)
    assert sa.pair_hard_negatives(20, 30, [1], [2], 1, 2, 1, np.zeros((20, 1024), F32), np.zeros((30, 1024), F32), W[2]).shape == (1,)


# ---- the stand-alone tool over the host-only header
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairhard_tool") / "check_pairhard_lists")
    subprocess.run(["c++", "-std=c++17", "-O1", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "svdfeature_amd", "csrc"),
                    os.path.join(ROOT, "tools", "check_pairhard_lists.cpp"), "-o", exe], check=True)
    return exe


def test_the_stand_alone_tool(tool):
    """built plain here; its header comment gives the sanitizer line for running it by hand"""
    out = subprocess.run([tool], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("m,C,k", [(1, 8, 7), (2, 3, 16), (1, 100, 5)])
def test_the_tools_negatives_are_numpys(tool, m, C, k):
    rng = np.random.default_rng(k)
    nu, ni, n = 40, 90, 300
    u, p = rng.integers(0, nu, n).astype(np.uint32), rng.integers(0, ni, n).astype(np.uint32)
    W = (rng.standard_normal((nu, k)).astype(F32), rank_rounding.cluster(rng, ni, k, 30), (1e-6 * rng.standard_normal(ni)).astype(F32))
    seed = (1 << 63) + 9
    text = "%d %d %d %d %d %d %d\n" % (nu, ni, n, m, C, seed, k) + "".join("%d %d\n" % (a, b) for a, b in zip(u, p))
    text += "".join(" ".join("%08x" % x for x in a.ravel().view(np.uint32)) + "\n" for a in W)
    out = subprocess.run([tool, "dump"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    got = {line.split()[0]: line.split()[1:] for line in out}
    neg, score = hard.rule_hard(nu, ni, u, p, m, C, seed, *W)
    assert np.array_equal(np.array(got["neg"], np.int64), neg)
    assert np.array_equal(np.array([int(x, 16) for x in got["score"]], np.uint32), score.view(np.uint32))
    refused = subprocess.run([tool, "dump"], input=text.replace(" %d %d %d %d\n" % (m, C, seed, k), " 2 129 %d %d\n" % (seed, k), 1),
                             capture_output=True, text=True, check=True).stdout
    assert refused.strip() == "refused pair_source: num_neg * num_cand must be at most 256"

"""The inputs of tests/test_gpu_float_edges.py, proven on the CPU: for every (route shape, stratum) the GPU tests run, the oracle alone must
show that the input reaches the float edge it is named after AND that a port which got that edge wrong would give other bits.  The shares below
are conditions on the inputs, not measurements of the code under test; seeds and sizes in tests/float_edges.py are chosen so that they hold.

  denormal, tiny_mixed  >= 10 % of the final factor values denormal, none NaN; the same run with flush-to-zero and denormals-are-zero set
                        (oracle.set_flush) differs in >= 10 % of them: the decoy a flushing kernel would match
  zeros                 both zero signs in the final factors; thresholded and surviving elements >= 10 % each; the run from the model whose -0
                        are +0 differs.  Where the item side decays by a factor (reg_method 3) it differs in a row the pass trains (float_edges:
                        the all -0 item row against the all +0 user row); under an L1 threshold on both sides (1, 5) every trained -0 is rewritten
                        to +0 by `else w = 0`, so there the difference sits in the untouched rows, which the engine must leave as they are
  overflow              an infinity and a NaN in the final model or the predictions, >= half of all values finite, and a finite value outside the
                        huge rows themselves that differs from the run in which they are of ordinary scale
  saturated_link        pre-link sums on each side of both thresholds of expf(-x) -- overflow at x < -88.72, results denormal for x > 87.34 and 0
                        for x > 103.97 -- and, where the predictions are linked (active_type 1, 2), exact 0, exact 1 and values between

The results are cached in float_edges, where the GPU tests find them.  With the compiled reference present, the restatement's own edge
behaviour is pinned to it on every case the reference's base solver covers."""
import os

import numpy as np
import pytest

import float_edges as fe
from oracle import oracle

RUNS = {}
for _r in fe.ROUTES:
    RUNS.setdefault((_r.key, _r.how, tuple(sorted(_r.kw.items()))), _r)
RUNS = sorted(RUNS.values(), key=lambda r: r.id)


def _share(mask):
    return float(np.mean(mask))


@pytest.mark.parametrize("route", RUNS, ids=lambda r: r.id)
def test_the_input_reaches_its_edge_and_tells_a_wrong_port_apart(route):
    c = route.case
    res = route.expected()
    fa, init = fe.factors(res), fe.factors(c.model)
    cl = fe.classes(fa)
    s = c.stratum
    if s in ("denormal", "tiny_mixed"):
        assert cl["nan"] == 0 and fe.classes(fe.everything(res))["nan"] == 0
        assert cl["denormal"] >= 0.10 * cl["n"], cl
        flushed = fe.expected(c, route.how, flush=True, **route.kw)
        assert fe.count_different(fa, fe.factors(flushed)) >= 0.10 * cl["n"]
        if c.shape != "big":   # (2^20 ratings: not a third time)
            assert not fe.count_different(fa, fe.factors(fe.expected(c, route.how, tag="again", **route.kw))), "the flush switch was left on"
    elif s == "zeros":
        assert cl["pos_zero"] > 0 and cl["neg_zero"] > 0 and cl["nan"] == 0, cl
        assert _share((fa == 0) & (init != 0)) >= 0.10 and _share((fa != 0) & (init != 0)) >= 0.10
        plus = fe.expected(c, route.how, model=fe.model_without_negative_zeros(c), tag="plus0", **route.kw)
        assert fe.count_different(fa, fe.factors(plus)) > 0
        if c.variant == 3 and route.how == "exact" and c.extend == 0:   # (nested spans: the row meets the open levels' feedback sums too)
            row = c.ni + 7
            assert np.signbit(res["W_item"][row]).any() and fe.count_different(res["W_item"][row], plus["W_item"][row]) > 0
    elif s == "overflow":
        al = fe.classes(fe.everything(res))
        assert al["pos_inf"] + al["neg_inf"] > 0 and al["nan"] > 0, al
        assert al["finite"] >= 0.5 * al["n"], al
        # the huge rows were read: a finite value OUTSIDE them -- a sink's or an ordinary row's -- differs from the run in which they are ordinary
        small = fe.expected(c, route.how, model=fe.model_without_huge_rows(c), tag="small", **route.kw)
        special = {"W_user": c.nu, "u_bias": c.nu, "W_item": c.ni, "i_bias": c.ni}
        moved = 0
        for name in c.model:
            a, b = res[name].copy(), small[name].copy()
            if name in special:
                a[special[name]:special[name] + 4] = b[special[name]:special[name] + 4] = 0
            both = np.isfinite(a) & np.isfinite(b)
            moved += int((a[both] != b[both]).sum())
        assert moved > 0
    else:
        assert s == "saturated_link"
        assert cl["nan"] == 0 and fe.classes(res["pred"])["nan"] == 0
        # the sums before the link, on the model the pass starts from: the same arrays under the linear link and no base score
        lin = fe.Case(**dict(c.__dict__, active=0, conf=[(k, v) for k, v in c.conf if k not in ("active_type", "base_score")] + [("base_score", "0")]))
        o = fe.fresh(lin, fe._port)
        x = fe.scores(o, lin)
        o.close()
        for lo, hi in ((-np.inf, -104.0), (-103.9, -88.8), (-88.7, -80.0), (80.0, 87.3), (87.4, 103.9), (104.0, np.inf)):
            assert ((x > lo) & (x < hi)).any(), (lo, hi)
        if c.active in (1, 2):
            p = res["pred"]
            assert (p == 0).any() and (p == 1).any() and ((p > 0) & (p < 1)).any()


REFERENCE_COVERS = [r for r in RUNS if r.how == "exact" and r.key[0] not in ("nested", "big")]   # (the base solver; 2^20 ratings: not twice)


@pytest.mark.skipif(not oracle.have_reference(), reason="the compiled reference is not present")
@pytest.mark.parametrize("route", REFERENCE_COVERS, ids=lambda r: r.id)
def test_the_restatement_equals_the_compiled_reference_at_the_edges(route, tmp_path):
    """the reference's shim cannot set a view: the arrays travel as a model file the restatement writes"""
    c = route.case
    path = os.path.join(str(tmp_path), "edge.model")
    p = fe.fresh(c, fe._port)
    p.save_model(path)
    p.close()
    r = oracle.OracleTrainer("reference", c.fmt, c.active, c.extend)
    r.seed(7)
    for name, v in c.conf:
        r.set_param(name, v)
    r.load_model(path)
    r.init_trainer()
    fe.train(r, c, **route.kw)
    got, want = fe.collect(r, c), route.expected()
    for name in want:
        fe.same_bits_or_nan(want[name], got[name], "%s of the restatement against the compiled reference" % name)
    r.close()


def test_same_bits_or_nan_is_strict_about_everything_but_nan_bits():
    a = np.array([0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan, 1.0], np.float32)
    b = a.copy()
    b.view(np.uint32)[5] = 0xffc00000
    fe.same_bits_or_nan(a, b)
    for at, v in ((0, -0.0), (1, 0.0), (2, 0.0), (2, 1.0001e-40), (3, 3.4e38), (4, np.nan), (5, 1.0), (6, np.nextafter(np.float32(1), np.float32(2)))):
        c = a.copy()
        c[at] = v
        with pytest.raises(AssertionError):
            fe.same_bits_or_nan(c, a)

"""CPU anchors of the asymmetric schedule-form cases (tests/forms_cases.py; the GPU side is tests/test_gpu_schedule_forms.py).

1. On every case, at a small size, the oracle port equals the compiled reference bit for bit after every round: the GPU tests' expectations are the
   reference's own numbers, not only the port's.
2. A plain float64 restatement of update_inner on (user:1, item:1), linear link, reg_method 0, written from the reference's order
   (apex_svd_base.h:456-462; oracle/svdf_oracle.c: pred, update_no_decay, regularize after the update), shares no code with the port: after one
   pass the port must lie within a stated float32 rounding margin of it, and the restatement with the two sides' decays exchanged at least 10x
   further away -- the asymmetric semantics themselves, checked independently.
"""
import numpy as np
import pytest

import cases
import forms_cases as fc
from oracle import oracle


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.skipif(not oracle.have_reference(), reason="compiled reference (oracle/_ref) not present")
@pytest.mark.parametrize("case", fc.ALL, ids=[c["name"] for c in fc.ALL])
def test_port_equals_the_compiled_reference(case):
    data, (nu, ni) = fc.make_data(case, scale=0.05)
    csr = fc.as_csr(data)
    for (r, a), (_, b) in zip(fc.checker_rounds("port", case, data, nu, ni), fc.checker_rounds("reference", case, data, nu, ni)):
        va, vb = fc.views(a), fc.views(b)
        for name in fc.NAMES:
            if va[name] is None or vb[name] is None:
                continue
            assert _same(va[name], vb[name]), (case["name"], "round", r, name)
        assert _same(a.predict_batch(csr), b.predict_batch(csr)), (case["name"], "round", r)


def _float64_pass(W_user, W_item, u_bias, i_bias, u, i, label, base, lr, wd_user, wd_item, wd_user_bias, wd_item_bias):
    P, Q = W_user.astype(np.float64), W_item.astype(np.float64)
    bu, bi = u_bias.astype(np.float64), i_bias.astype(np.float64)
    for uu, ii, y in zip(u.tolist(), i.tolist(), label.astype(np.float64).tolist()):
        p, q = P[uu].copy(), Q[ii].copy()
        err = y - (base + bu[uu] + bi[ii] + float(p @ q))
        P[uu] = (p + lr * err * q) * (1.0 - lr * wd_user)
        Q[ii] = (q + lr * err * p) * (1.0 - lr * wd_item)
        bu[uu] = (bu[uu] + lr * err) * (1.0 - lr * wd_user_bias)
        bi[ii] = (bi[ii] + lr * err) * (1.0 - lr * wd_item_bias)
    return {"W_user": P, "W_item": Q, "u_bias": bu, "i_bias": bi}


# Calibrated on this data (largest difference over the four arrays, relative to the array's largest entry): the port (float32 rows, the bias sum
# and dot accumulated in double) sits 0.9e-6 .. 1.7e-6 from the float64 restatement; with the decays exchanged the restatement lies 3e-2 .. 7e-2
# away.  TOL is about 10x the float32 distance and 1/1000 of the mirrored one.
TOL = 2e-5


@pytest.mark.parametrize("decay", fc.DECAYS[:3])
def test_port_follows_a_float64_restatement_of_the_asymmetric_step(decay):
    nu, ni, n, k, lr, base = 300, 50, 4000, 16, 0.02, 1.7
    wd_user, wd_item, wd_user_bias, wd_item_bias = decay
    u, i, r = cases.planted_triples(n, nu, ni, seed=5)
    y = fc.labels(r, 0, 5)
    o = oracle.OracleTrainer("port", 0, 0)
    o.seed(10)
    for kk, v in [("num_user", nu), ("num_item", ni), ("num_global", 0), ("num_factor", k), ("active_type", 0), ("base_score", base),
                  ("learning_rate", lr), ("wd_user", wd_user), ("wd_item", wd_item), ("wd_user_bias", wd_user_bias), ("wd_item_bias", wd_item_bias)]:
        o.set_param(kk, str(v))
    o.init_model()
    o.init_trainer()
    init = fc.views(o)
    o.update_batch(cases.CSRData.from_triples(u, i, y))
    got = fc.views(o)
    args = (u, i, y, base, lr)
    direct = _float64_pass(init["W_user"], init["W_item"], init["u_bias"], init["i_bias"], *args, wd_user, wd_item, wd_user_bias, wd_item_bias)
    mirror = _float64_pass(init["W_user"], init["W_item"], init["u_bias"], init["i_bias"], *args, wd_item, wd_user, wd_item_bias, wd_user_bias)

    def dist(ref):
        return max(float(np.max(np.abs(got[nm].astype(np.float64) - ref[nm]))) / max(float(np.max(np.abs(ref[nm]))), 1e-30) for nm in fc.NAMES)
    d_direct, d_mirror = dist(direct), dist(mirror)
    print("float64 distance: direct %.3g, mirrored %.3g" % (d_direct, d_mirror))
    assert d_direct <= TOL, d_direct
    assert d_mirror >= 10 * d_direct and d_mirror >= 10 * TOL, (d_direct, d_mirror)

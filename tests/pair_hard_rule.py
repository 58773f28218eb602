"""The rule of a HARD pass of a pair source (include/svdfeature_amd.h) in numpy -- written from the published statement, not
from the C++ (helper of tests/test_pair_hard.py and tests/test_gpu_pair_hard.py; not collected).

    num_neg = m pairs per row, num_cand = C candidates per pair; pair q = r * m + j of row (user_r, pos_r)
    cand(q, i) = the plain rule's negative of pair index q * C + i in a pass with m * C negatives per row and the same seed
    score(q, i) = the ranker's float32 score of (user_r, cand(q, i)): rank_rounding.score_fp32
    neg_q      = the non-NaN candidate with the highest score, -0 counting as +0, equal scores to the smaller id; all NaN: cand(q, 0)"""
import numpy as np

import pair_source_rule
import rank_rounding

F32 = np.float32


def candidates(num_user, num_item, user, pos_item, num_neg, num_cand, seed):
    """int64 [n * num_neg, num_cand]"""
    m, C = int(num_neg), int(num_cand)
    return pair_source_rule.rule_negatives(num_user, num_item, user, pos_item, m * C, seed).astype(np.int64).reshape(-1, C)


def scores(cand, user, num_neg, W_user, W_item, i_bias, order="pinned"):
    """float32 [n * num_neg, num_cand]: one score_fp32 call per distinct user over the candidates of all its pairs"""
    out = np.zeros(cand.shape, F32)
    W_user, W_item, i_bias = np.asarray(W_user, F32), np.asarray(W_item, F32), np.asarray(i_bias, F32)
    owner = np.repeat(np.asarray(user, np.int64), int(num_neg))
    with np.errstate(all="ignore"):
        for u in np.unique(owner):
            mine = owner == u
            c = cand[mine].ravel()
            out[mine] = rank_rounding.score_fp32(W_user[u], W_item[c], i_bias[c], order).reshape(-1, cand.shape[1])
    return out


def select(cand, sc):
    """(chosen id uint32 [n * num_neg], chosen score float32, pairs whose two best keys differ in score: the choice hangs on no tie)"""
    s = sc.astype(np.float64)        # exact, and -0.0 == 0.0 sorts as one value
    s = np.where(s == 0, 0.0, s)
    nan = np.isnan(s)
    key = np.where(nan, -np.inf, s)  # a NaN is never chosen while another exists: below every score, and excluded from ties below
    # lexsort per row: by score descending, then id ascending; NaN entries last
    order = np.lexsort((cand, -key, nan), axis=1)
    at = order[:, 0]
    rows = np.arange(len(cand))
    all_nan = nan.all(axis=1)
    at = np.where(all_nan, 0, at)
    chosen, chosen_score = cand[rows, at], sc[rows, at]
    if cand.shape[1] > 1:
        second = order[:, 1]
        untied = ~all_nan & (nan[rows, second] | (key[rows, second] != key[rows, at]) | (cand[rows, second] == chosen))
    else:
        untied = np.ones(len(cand), bool)
    return chosen.astype(np.uint32), chosen_score, untied


def rule_hard(num_user, num_item, user, pos_item, num_neg, num_cand, seed, W_user, W_item, i_bias, order="pinned", full=False):
    """(negatives, chosen scores) of the rule; full: also (candidates, scores, untied)"""
    cand = candidates(num_user, num_item, user, pos_item, num_neg, num_cand, seed)
    sc = scores(cand, user, num_neg, W_user, W_item, i_bias, order)
    neg, chosen, untied = select(cand, sc)
    return (neg, chosen, cand, sc, untied) if full else (neg, chosen)


def same_scores(a, b):
    """bit for bit, a NaN equal to any NaN (the sign and payload of a NaN score are not specified)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---- the inputs the CPU and the GPU tests share
NU, NI, N = 200, 300, 3000
SHAPES = [(1, 1), (1, 2), (1, 7), (1, 8), (2, 3), (3, 5), (4, 64), (1, 65), (1, 100), (1, 256)]   # (num_neg, num_cand)


def rows(order, n=N, seed=5):
    """n positives of 200 users x 300 items with repeated (user, item) rows; users 0 and 1 have no row, user 2 has one"""
    rng = np.random.default_rng(seed)
    u = rng.integers(3, NU, n)
    u[0] = 2
    p = rng.integers(0, NI, n)
    p[n // 2:n // 2 + 20], u[n // 2:n // 2 + 20] = p[:20], u[:20]
    if order == "grouped":
        at = np.argsort(u, kind="stable")
        u, p = u[at], p[at]
    return u.astype(np.uint32), p.astype(np.uint32)


def model(k, seed=0):
    rng = np.random.default_rng(100 * k + seed)
    return rng.standard_normal((NU, k)).astype(F32), rng.standard_normal((NI, k)).astype(F32), (0.1 * rng.standard_normal(NI)).astype(F32)


def tie_model(k=6):
    """items c and c + 150 have one row and one bias: equal scores, the smaller id wins"""
    Wu, Wi, b = model(k, seed=1)
    Wi[NI // 2:], b[NI // 2:] = Wi[:NI // 2], b[:NI // 2]
    return Wu, Wi, b


def zero_model(k=5):
    """a zero user matrix, biases +0 and -0: every score ties"""
    Wu, Wi, b = model(k, seed=2)
    Wu[:] = 0
    b[:] = np.where(np.arange(NI) % 2 == 1, F32(0.0), F32(-0.0))
    return Wu, Wi, b


def nan_model(k=9):
    """every third item row holds a NaN; user 5's row is all NaN, user 7's has one in the tail: every score of theirs is NaN"""
    Wu, Wi, b = model(k, seed=3)
    Wi[np.arange(0, NI, 3), np.arange(0, NI, 3) % k] = np.nan
    Wu[5], Wu[7, k - 1] = np.nan, np.nan
    return Wu, Wi, b


def inf_model(k=4):
    """every fifth bias is +inf or -inf"""
    Wu, Wi, b = model(k, seed=4)
    b[np.arange(0, NI, 10)] = -np.inf
    b[np.arange(5, NI, 10)] = np.inf
    return Wu, Wi, b


def rounding_model(k):
    """rank_rounding.cluster: the item rows are one base row plus perturbations of +-30 ulp per element, so a pair's eight scores lie a few ulp
    of the score apart"""
    rng = np.random.default_rng(7000 + k)
    return rng.standard_normal((NU, k)).astype(F32), rank_rounding.cluster(rng, NI, k, 30), (1e-6 * rng.standard_normal(NI)).astype(F32)

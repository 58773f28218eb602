"""(not collected by pytest) Shared by the tests of the ordered sub-steps for hot items of rank pairs in the window step (knob
`window_pair_sub`; svdf_wseq.cpp: wseq_from_pairs, svdf_k_window.hip: k_window_apply_pairs): the pair draws, what a
draw holds window by window and the checker call.  (The window rule: tests/window_rule.py, columns with both items of a pair counted.)

The checker is tests/window_sim.py on the pair-shaped rows of svdfeature_amd.pairs_as_csr -- no global entry, user:1, the two item entries
in ascending id with the negative's sign flipped, label 1 -- with B = num_user (no shared user row), no tables and isub = window_pair_sub."""
import numpy as np

import cases
import svdfeature_amd as sa
import window_sim as ws

NU, NI = 60, 40
HOT = (0, 1, 2)
VIEWS = ("W_user", "u_bias", "W_item", "i_bias")


def conf(k, active=3, reg=0, extra=(), nu=NU, ni=NI):
    c = cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_global=0, num_factor=k, reg_method=reg, learning_rate="0.01",
                        active_type=active) + list(extra)
    return cases.conf_with(c, base_score="0.5") if active != 0 else c


def ip_ranges(ni=NI):
    """per-id item decay ranges that split the hot items 0 .. 2"""
    return (("ip:wd", "0.01"), ("ip:bound", "2"), ("ip:wd", "0.003"), ("ip:bound", str(ni // 2)), ("ip:wd", "0.02"), ("ip:bound", str(ni)))


def draw_pairs(rng, n, p_pos=0.8, p_neg=0.3, hot=HOT, nu=NU, ni=NI):
    """(user, positive, negative): the positive item is a hot one with probability p_pos, the negative with p_neg; pos != neg"""
    u = rng.integers(0, nu, n).astype(np.uint32)
    cold = [i for i in range(ni) if i not in hot]

    def one(p):
        return int(rng.choice(hot)) if hot and rng.random() < p else int(rng.choice(cold))
    pos, neg = np.empty(n, np.uint32), np.empty(n, np.uint32)
    for r in range(n):
        a = one(p_pos)
        b = one(p_neg)
        while b == a:
            b = one(p_neg)
        pos[r], neg[r] = a, b
    return u, pos, neg


def facts(pos, neg, W, s):
    """what the pairs hold, window by window (the cuts of wseq_from_pairs): hot rows, a ragged last sub-step, pairs with two hot items, a hot
    item met as the lower / higher id and as positive / negative"""
    f = dict(nhot=0, ragged=False, two_hot=0, as_lo=False, as_hi=False, as_pos=False, as_neg=False, most=0)
    n = len(pos)
    for b0, b1 in ws.row_cuts(n, W):
        cnt = np.bincount(np.concatenate([pos[b0:b1], neg[b0:b1]]).astype(np.int64))
        hot = {int(i) for i in np.nonzero(cnt > s)[0]}
        f["nhot"] += len(hot)
        f["ragged"] = f["ragged"] or any(cnt[i] % s for i in hot)
        f["most"] = max([f["most"]] + [int(cnt[i]) for i in hot])
        for r in range(b0, b1):
            a, b = int(pos[r]), int(neg[r])
            f["two_hot"] += a in hot and b in hot
            for x, other in ((a, b), (b, a)):
                if x in hot:
                    f["as_lo" if x < other else "as_hi"] = True
            f["as_pos"] = f["as_pos"] or a in hot
            f["as_neg"] = f["as_neg"] or b in hot
    return f


def check(c, u, pos, neg, W, passes, s, **kw):
    """the checker's model after `passes` passes of W windows; s = 0: the plain window step"""
    d = sa.pairs_as_csr(u, pos, neg)
    active = int(dict(c).get("active_type", 0))
    ub = dict(c).get("no_user_bias", "0") != "1"
    nu = int(dict(c)["num_user"])
    o = ws.make_oracle(c, active=active)
    if s == 0:
        return ws.simulate_rows(o, d, nu, W, passes, fu=(), fi=(), user_bias=ub)
    return ws.simulate_rows(o, d, nu, W, passes, isub=s, user_bias=ub, **kw)

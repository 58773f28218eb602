"""Asymmetric configurations of the engine's exact schedule forms, shared by the GPU tests (tests/test_gpu_schedule_forms.py: engine == C oracle
bit for bit, route asserted) and the CPU anchors (tests/test_schedule_forms_cpu.py: oracle port == compiled reference on the same cases).

The forms' older tests all run with wd_user == wd_item, zero bias decays, a fixed learning rate and the linear link, where swapping or dropping the
two sides' decays changes nothing.  Every case here has different row decays (one of them 0 in some: the snap-to-one path), different nonzero bias
decays, a learning rate other than 0.005 decayed by 0.9 per round, a base score other than 3 and real-valued labels with negatives (0/1 labels for
the sigmoid links).

    form            ds.kind  counter  route knobs
    runs            10       23       runs_exec = 1, pivot_exec = 0, runs_min_rows = 0   (svdf_runs.cpp, k_basicmf_runs_soa)
    hot-row units   9        22       pivot_exec = 1, runs_exec = 0                       (svdf_pivot.cpp, k_svdpp_wave + the contract kernel)
    pair units      11       29       pair_units = 1                                      (svdf_punit.cpp, k_pair_units)
    plain levels    0        -        runs_exec = 0, pivot_exec = 0                       (control)
"""
import numpy as np

import cases
import svdfeature_amd as sa

NAMES = ("W_user", "W_item", "u_bias", "i_bias")
COUNTER = {10: 23, 9: 22, 11: 29}
SIGMOID = {1, 2, 3, 7}

# (wd_user, wd_item, wd_user_bias, wd_item_bias): never symmetric; a zero row decay runs the snap path (a decay factor of exactly 1)
DECAYS = [(0.02, 0.0, 0.01, 0.003), (0.0, 0.03, 0.002, 0.02), (0.004, 0.05, 0.05, 0.001), (0.03, 0.002, 0.004, 0.03)]
LRS = (0.01, 0.02, 0.007)


def _case(name, kind, k, active, data, decay, lr, knobs, rounds, extra=()):
    wu, wi, wub, wib = decay
    base = 0.3 if active in SIGMOID else (0.5 if kind == 11 else (1.7 if active == 0 else 0.4))
    conf = [("num_global", 0), ("num_factor", k), ("active_type", active), ("base_score", base), ("learning_rate", lr),
            ("wd_user", wu), ("wd_item", wi), ("wd_user_bias", wub), ("wd_item_bias", wib), ("decay_learning_rate", 1), ("decay_rate", 0.9)]
    return dict(name=name, kind=kind, k=k, active=active, data=data, conf=conf + list(extra), knobs=list(knobs), rounds=rounds)


def _runs_cases():
    out, j = [], 0
    shapes = [("uniform", 6000, 800, 80000), ("zipf", 5000, 300, 60000), ("repeats", 400, 60, 20000)]
    for k in (64, 128):
        for rl in (2, 4, 7):
            for sets in (1, 2):
                shape = shapes[j % 3]
                knobs = [("runs_exec", 1), ("pivot_exec", 0), ("runs_min_rows", 0), ("runs_len", rl), ("runs_sets", sets),
                         ("runs_block", (64, 128, 256)[j % 3])]
                out.append(_case("runs_k%d_len%d_sets%d_%s" % (k, rl, sets, shape[0]), 10, k, 0, shape + (100 + j,), DECAYS[j % 4],
                                 LRS[j % 3], knobs, 2 + j % 2))
                j += 1
    return out


def _pivot_cases():
    # (k, link, hot side, pivot_min, pivot_run)
    rows = [(1, 0, "item_hot", 2, 256), (3, 3, "user_hot", 256, 2), (16, 1, "item_hot", 64, 8), (33, 5, "user_hot", 1000, 64),
            (64, 0, "user_hot", 256, 2), (64, 2, "item_hot", 256, 256), (100, 0, "item_hot", 500, 16), (128, 3, "item_hot", 64, 2),
            (200, 5, "item_hot", 256, 32), (256, 0, "user_hot", 128, 256), (256, 1, "item_hot", 2, 2), (33, 0, "item_hot", 256, 7)]
    out = []
    for j, (k, act, side, pmin, prun) in enumerate(rows):
        data = (side, 4000, 200, 50000, 200 + j) if side == "item_hot" else (side, 200, 4000, 50000, 200 + j)
        knobs = [("pivot_exec", 1), ("runs_exec", 0), ("pivot_min", pmin), ("pivot_run", prun)]
        out.append(_case("pivot_k%d_link%d_%s_min%d_run%d" % (k, act, side, pmin, prun), 9, k, act, data, DECAYS[j % 4], LRS[j % 3], knobs,
                         2 + j % 2))
    return out


def _pair_cases():
    # (reg_method, no_user_bias, k, unit cap)
    rows = [(0, 1, 16, 16), (0, 0, 64, 5), (1, 1, 128, 24), (1, 0, 200, 16), (2, 1, 64, 64), (2, 0, 16, 16), (3, 1, 200, 7), (3, 0, 128, 16)]
    out = []
    for j, (reg, nub, k, cap) in enumerate(rows):
        decay = DECAYS[j % 4]
        if reg == 2:   # project(): wd is a bound on the row's squared norm; small enough to bind on both sides
            decay = (0.002, 0.0007) + decay[2:]
        extra = [("reg_method", reg), ("no_user_bias", nub)]
        out.append(_case("pairs_reg%d_nub%d_k%d_cap%d" % (reg, nub, k, cap), 11, k, 3, ("pairs", 150, 600, 60, 300 + j), decay, LRS[j % 3],
                         [("pair_units", 1), ("pair_unit_cap", cap)], 2 + j % 2, extra))
    return out


def _plain_cases():
    rows = [(8, 0, 0, "zipf"), (64, 4, 1, "uniform"), (256, 0, 0, "repeats"), (64, 0, 5, "zipf")]
    out = []
    for j, (k, cw, act, shape) in enumerate(rows):
        data = {"uniform": ("uniform", 3000, 500, 40000), "zipf": ("zipf", 3000, 200, 40000), "repeats": ("repeats", 300, 40, 12000)}[shape]
        knobs = [("runs_exec", 0), ("pivot_exec", 0), ("chain_width", cw)]
        out.append(_case("plain_k%d_chain%d_link%d_%s" % (k, cw, act, shape), 0, k, act, data + (400 + j,), DECAYS[(j + 1) % 4], LRS[j % 3],
                         knobs, 2 + j % 2))
    return out


RUNS = _runs_cases()
PIVOT = _pivot_cases()
PAIRS = _pair_cases()
PLAIN = _plain_cases()
ALL = RUNS + PIVOT + PAIRS + PLAIN


def labels(r, active, seed):
    """real-valued labels around the planted ratings, some negative (linear / hinge-free links); 0/1 for the sigmoid and hinge links"""
    if active != 0:
        return (r > 3).astype(np.float32)
    rng = np.random.default_rng(seed)
    return (r + rng.uniform(-0.5, 0.5, len(r)) - 2.25).astype(np.float32)


def make_data(case, scale=1.0):
    """("triples", u, i, r) or ("pairs", u, p, q), plus (num_user, num_item); scale < 1 shrinks the data set (the CPU anchors)"""
    shape, nu, ni, n, seed = case["data"]
    if shape == "pairs":
        per = max(4, int(n * scale))
        rng = np.random.default_rng(seed)
        u = np.repeat(rng.permutation(nu).astype(np.uint32), per)
        cut = rng.integers(0, len(u), max(1, len(u) // 50))   # some users' blocks broken up (tests/fuzz_punit.py)
        u[cut] = rng.integers(0, nu, len(cut)).astype(np.uint32)
        p = rng.integers(0, ni, len(u)).astype(np.uint32)
        q = ((p + 1 + rng.integers(0, ni - 1, len(u))) % ni).astype(np.uint32)
        return ("pairs", u, p, q), (nu, ni)
    n = max(500, int(n * scale))
    if shape == "repeats":   # the same (user, item) twice in a row and the same user on consecutive ratings (tests/test_gpu_runs.py)
        rng = np.random.default_rng(seed)
        u = rng.integers(0, nu, n).astype(np.uint32)
        i = rng.integers(0, ni, n).astype(np.uint32)
        u[1::7] = u[0::7][:len(u[1::7])]
        i[1::7] = i[0::7][:len(i[1::7])]
        r = rng.integers(1, 6, n).astype(np.float32)
    elif shape == "user_hot":   # Zipf-popular USERS: the walker on plain parameters
        i, u, r = cases.planted_triples(n, ni, nu, seed, zipf=True)
    else:
        u, i, r = cases.planted_triples(n, nu, ni, seed, zipf=shape in ("zipf", "item_hot"))
    return ("triples", u, i, labels(r, case["active"], seed)), (nu, ni)


def conf_of(case, nu, ni, mirrored=False):
    conf = [("num_user", nu), ("num_item", ni)] + list(case["conf"])
    if mirrored:   # the two sides' decays exchanged
        d = dict(conf)
        swap = {"wd_user": d["wd_item"], "wd_item": d["wd_user"], "wd_user_bias": d["wd_item_bias"], "wd_item_bias": d["wd_user_bias"]}
        conf = [(k, swap.get(k, v)) for k, v in conf]
    return conf


def as_csr(data):
    return sa.pairs_as_csr(*data[1:]) if data[0] == "pairs" else sa.CSRData.from_triples(*data[1:])


def setup(t, case, nu, ni, mirrored=False):
    t.seed(10)
    for k, v in conf_of(case, nu, ni, mirrored):
        t.set_param(k, str(v))
    t.init_model()
    t.init_trainer()
    return t


def checker(kind, case, nu, ni, mirrored=False):
    """an OracleTrainer ("port" / "reference") set up for the case"""
    from oracle import oracle
    return setup(oracle.OracleTrainer(kind, 0, case["active"]), case, nu, ni, mirrored)


def checker_rounds(kind, case, data, nu, ni, mirrored=False):
    """the CPU checker trained round by round: yields (round, trainer) after each round"""
    o = checker(kind, case, nu, ni, mirrored)
    csr = as_csr(data)
    for r in range(case["rounds"]):
        o.set_round(r)
        o.update_batch(csr)
        o.finish_round()
        yield r, o


def views(t):
    out = {}
    for n in NAMES:
        v = t.view(n)
        out[n] = None if v is None else np.array(v, np.float32, copy=True)
    return out

"""Inputs on which the ranker's integer results depend on the last bit of a score, and the arithmetic contract of DESIGN.md 4c restated in
numpy float32 (helper of tests/test_rank_rounding.py and tests/test_gpu_ranker_rounding.py; not collected).

The candidates of a case are one base row plus perturbations of a few hundred ulp per element, so the scores of a section lie a few ulp of
the SCORE apart and any other order of the same additions moves ranks.  `Case.scores()` restates the contract (unfused axpy in feature order for the
prepared rows and the user sum, the bias as a float sum, four serial chains over the 4-float chunks, (a0 + a2) + (a1 + a3), the tail in index
order, bias + sum) and, by name, the DECOYS: the orders a kernel could use by mistake.  The models are written through the C oracle's trainer
(set_view + save_model), so nothing here needs a GPU."""
import numpy as np

import cases
from oracle import oracle
from svdfeature_amd.data import CSRData, PlusBlock

F32 = np.float32
F64 = np.float64

DOT_DECOYS = ("sequential", "pair01", "serial4", "fma", "eight")
DECOYS = DOT_DECOYS + ("fused_prep", "fused_user")


def _madd(acc, a, b, fused):
    """acc + a * b: two roundings, or (decoy) product and sum in float64 and one rounding to float32"""
    if fused:
        return (acc.astype(F64) + np.asarray(a, F64) * np.asarray(b, F64)).astype(F32)
    return acc + a * b


def dot_fp32(urow, W, order="pinned"):
    """sdot of every row of W with urow in float32, in the pinned order or a decoy's"""
    n, k = W.shape
    if order == "sequential":
        s = np.zeros(n, F32)
        for t in range(k):
            s = s + urow[t] * W[:, t]
        return s
    fused = order == "fma"
    nfull = k // 4
    a = np.zeros((n, 4), F32)
    b = np.zeros((n, 4), F32)          # the second accumulator set of the eight-chain decoy
    for j in range(nfull):
        m = (urow[4 * j:4 * j + 4][None, :], W[:, 4 * j:4 * j + 4])
        if order == "eight" and j % 2:
            b = _madd(b, *m, False)
        else:
            a = _madd(a, *m, fused)
    if order == "eight":
        a = a + b
    if order == "pair01":
        s = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
    elif order == "serial4":
        s = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
    else:
        s = (a[:, 0] + a[:, 2]) + (a[:, 1] + a[:, 3])
    for t in range(4 * nfull, k):
        s = _madd(s, urow[t], W[:, t], fused)
    return s


def score_fp32(urow, W, bias, order="pinned"):
    """the ranker's score in numpy float32: four chains over the 4-float chunks, (a0 + a2) + (a1 + a3), the tail in index order, bias + sum"""
    return F32(0.0) + (bias + dot_fp32(urow, W, order))


def feature_sum(W, idx, val, start=None, fused=False):
    """rows f = start (or 0); f = f + W[idx[:, j]] * val[:, j] for j in feature order -- the prepared candidate rows and the user sum"""
    idx, val = np.atleast_2d(idx), np.atleast_2d(np.asarray(val, F32))
    f = np.zeros((idx.shape[0], W.shape[1]), F32) if start is None else np.array(start, F32, ndmin=2)
    for j in range(idx.shape[1]):
        f = _madd(f, W[idx[:, j]], val[:, j][:, None], fused)
    return f


def bias_sum(b, idx, val):
    """bias = bias + b[idx] * val in float32, in feature order"""
    idx, val = np.atleast_2d(idx), np.atleast_2d(np.asarray(val, F32))
    out = np.zeros(idx.shape[0], F32)
    for j in range(idx.shape[1]):
        out = out + b[idx[:, j]] * val[:, j]
    return out


def cluster(rng, n, k, spread):
    """n rows: one standard normal base row plus integer perturbations of the bit patterns in +-spread"""
    base = rng.standard_normal(k).astype(F32)
    bits = np.tile(base.view(np.int32), (n, 1)) + rng.integers(-spread, spread + 1, (n, k)).astype(np.int32)
    return bits.view(F32)


class Case:
    """One model, its candidates and its user sections.

    builder "a": candidate c is the single feature (c, 1); W_item = base row + perturbations; biases of about 1e-6.  With `spec`, W_item holds a
    second cluster (rows ncand ..) and every section overrides a random half of the candidates by SPEC lines whose item feature is (ncand + c, 1).
    builder "b": candidate c is [(0, 0.37), (1 + c, 0.7319)]; row 0 is one base row, rows 1.. a second base row + perturbations, i_bias[1:] all
    equal; users are [(u0, 0.83), (u1, v)]: the products round, so a fused axpy in the preparation or in the user sum is visible.
    fmt 1: a user-group model; every group of sections arrives as one block with a feedback list of three entries.
    groups: the numbers of sections handed to the ranker per call (a call's sections form its tiles); npos: positives per section, or a function
    of the section's number; top_k 0 = positions mode."""

    def __init__(self, builder, k, ncand, groups, npos=5, top_k=0, nban=0, spec=False, fmt=0, spread=800, seed=0):
        self.builder, self.k, self.ncand, self.groups, self.top_k, self.nban, self.spec, self.fmt = builder, k, ncand, tuple(groups), top_k, nban, spec, fmt
        self.nsec = sum(groups)
        rng = np.random.default_rng(1000 * k + seed)
        self.nu = nu = 40
        c = np.arange(ncand)
        if builder == "a":
            self.W_item = cluster(rng, ncand, k, spread)
            if spec:
                self.W_item = np.concatenate([self.W_item, cluster(rng, ncand, k, spread)])
            self.i_bias = (1e-6 * rng.standard_normal(len(self.W_item))).astype(F32)
            self.cand_idx, self.cand_val = c[:, None], np.ones((ncand, 1), F32)
        else:
            self.W_item = np.concatenate([rng.standard_normal((1, k)).astype(F32), cluster(rng, ncand, k, spread)])
            self.i_bias = np.full(1 + ncand, F32(0.0123), F32)
            self.i_bias[0] = F32(0.31)
            self.cand_idx = np.stack([np.zeros(ncand, np.int64), 1 + c], 1)
            self.cand_val = np.tile(np.array([0.37, 0.7319], F32), (ncand, 1))
        self.ni = len(self.W_item)
        self.W_user = rng.standard_normal((nu, k)).astype(F32)
        self.nfb = 30 if fmt == 1 else 0
        self.W_ufb = (0.3 * rng.standard_normal((self.nfb, k))).astype(F32)
        self.sections = []
        for s in range(self.nsec):
            if builder == "a":
                uidx, uval = rng.integers(0, nu, 1), np.ones(1, F32)
            else:
                uidx, uval = rng.integers(0, nu, 2), np.array([0.83, rng.uniform(0.1, 1.0)], F32)
            perm = rng.permutation(ncand)
            n = npos(s) if callable(npos) else npos
            sec = dict(uidx=uidx, uval=uval, pos=perm[:n], ban=perm[n:n + nban], spec=np.sort(rng.permutation(ncand)[:ncand // 2]) if spec else perm[:0])
            self.sections.append(sec)
        self.feedback = [(np.sort(rng.choice(self.nfb, 3, replace=False)), rng.uniform(0.2, 0.9, 3).astype(F32)) for _ in self.groups] if fmt == 1 else []

    # ---- the model file and the input stream ----
    def write_model(self, path):
        kw = dict(num_user=self.nu, num_item=self.ni, num_factor=self.k)
        if self.fmt == 1:
            kw.update(num_ufeedback=self.nfb, ufeedback_init_sigma=0.05)
        t = oracle.OracleTrainer("port", self.fmt, 0)
        t.seed(1)
        for kk, v in cases.conf_with(cases.BASICMF_CONF, **kw):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        t.set_view("W_item", self.W_item)
        t.set_view("W_user", self.W_user)
        t.set_view("i_bias", self.i_bias)
        if self.fmt == 1:
            t.set_view("W_ufeedback", self.W_ufb)
        t.save_model(path)
        t.close()
        return path

    def items(self):
        return CSRData.from_rows([(0.0, [], [], [(int(i), float(v)) for i, v in zip(ii, vv)]) for ii, vv in zip(self.cand_idx, self.cand_val)])

    def section_rows(self, s):
        sec = self.sections[s]
        rows = [(2.0, [], [(int(i), float(v)) for i, v in zip(sec["uidx"], sec["uval"])], [])]
        if len(sec["pos"]):
            rows.append((1.0, [], [(int(x), 1.0) for x in sec["pos"]], []))
        if len(sec["ban"]):
            rows.append((-1.0, [], [(int(x), 1.0) for x in sec["ban"]], []))
        rows += [(3.0, [], [(int(x), 1.0)], [(self.ncand + int(x), 1.0)]) for x in sec["spec"]]
        rows.append((4.0, [], [], []))
        return rows

    def group_streams(self):
        out, s = [], 0
        for g in self.groups:
            out.append(CSRData.from_rows([row for j in range(s, s + g) for row in self.section_rows(j)]))
            s += g
        return out

    def run(self, make, path, how="rows", params=()):
        """the case through a ranker made by make(format_type): "rows" = one process_rows call per group of sections (one block per group for a
        user-group model), "lines" = one process call per line; returns the concatenated results and the ranker"""
        r = make(self.fmt)
        for kk, v in tuple(params) + (("top_k", str(self.top_k)),):
            r.set_param(kk, v)
        r.load_model(path)
        r.init_ranker(self.ncand)
        out = [r.process_rows(self.items())]
        assert out[0].size == 0
        for g, d in enumerate(self.group_streams()):
            if self.fmt == 1:
                out.append(r.process_block(PlusBlock(self.feedback[g][0], self.feedback[g][1], d, 0)))
            elif how == "lines":
                out += [r.process(*d.row(i)) for i in range(d.num_row)]
            else:
                out.append(r.process_rows(d))
        return np.concatenate(out).astype(np.int32), r

    # ---- the contract in numpy ----
    def decoys(self):
        """the decoys that CAN change this case's scores: without a full chunk every summation order is the tail's; eight chains equal four up to
        two chunks; a fused axpy shows only where the products round (builder b)"""
        d = ["fma"] if self.k < 4 else ["sequential", "pair01", "serial4", "fma"] + (["eight"] if self.k >= 12 else [])
        return d + (["fused_prep", "fused_user"] if self.builder == "b" else [])

    def scores(self, decoy="pinned"):
        """the final score of every candidate, per section"""
        order = decoy if decoy in DOT_DECOYS else "pinned"
        rows = feature_sum(self.W_item, self.cand_idx, self.cand_val, fused=decoy == "fused_prep")
        bias = bias_sum(self.i_bias, self.cand_idx, self.cand_val)
        out, s = [], 0
        for g, n in enumerate(self.groups):
            fb = feature_sum(self.W_ufb, self.feedback[g][0][None, :], self.feedback[g][1][None, :], fused=decoy == "fused_user") if self.fmt == 1 else None
            for sec in self.sections[s:s + n]:
                tu = feature_sum(self.W_user, sec["uidx"][None, :], sec["uval"][None, :], start=fb, fused=decoy == "fused_user")[0]
                first = np.zeros(self.ncand, F32)
                sp = sec["spec"]
                if len(sp):   # item_score = bias + sdot of the SPEC line's own prepared row
                    first[sp] = self.i_bias[self.ncand + sp] + dot_fp32(tu, self.W_item[self.ncand + sp], order)
                out.append(first + (bias + dot_fp32(tu, rows, order)))
            s += n
        return out

    def results(self, scores):
        """(results, sizes): positions mode -- the position of every positive, one output each; top_k mode -- the prefix of every section, top_k
        entries per output"""
        res = []
        ids = np.arange(self.ncand)
        for sec, sc in zip(self.sections, scores):
            on = np.ones(self.ncand, bool)
            on[sec["ban"]] = False
            if self.top_k:
                cid = ids[on]
                res.append(cid[np.lexsort((cid, -sc[on]))][:self.top_k])
            else:
                p = sec["pos"]
                eq = (sc[None, :] == sc[p][:, None]) & on[None, :] & (ids[None, :] < p[:, None])
                res.append(((sc[None, :] > sc[p][:, None]) & on[None, :]).sum(1) + eq.sum(1))
        return np.concatenate(res).astype(np.int32)

    def compared(self, scores):
        """one flag per output: untied in the given scores (a position: no other ranked candidate has the positive's score; a prefix: the
        top_k + 1 best ranked scores are pairwise distinct)"""
        flags = []
        for sec, sc in zip(self.sections, scores):
            on = np.ones(self.ncand, bool)
            on[sec["ban"]] = False
            if self.top_k:
                best = -np.sort(-sc[on])[:self.top_k + 1]
                flags.append(np.array([(np.diff(best) != 0).all()]))
            else:
                flags.append(np.array([(on & (sc == sc[p])).sum() == 1 for p in sec["pos"]], bool))
        return np.concatenate(flags)

    def per_output(self, flat):
        """the flat results as one row per output"""
        return flat.reshape(-1, self.top_k) if self.top_k else flat.reshape(-1, 1)


def many(s):
    return 70 if s == 1 else 20


POS_GROUPS = (37, 3)                       # tiles: NSEC 8 (a full tile of 32 and a ragged one of 5), then NSEC 4
TOP_GROUPS = (3, 7, 13) * 4                # tiles: NSEC 4, 8, 16
WIDTHS = (3, 5, 8, 12, 34, 64, 130, 300)   # no full chunk / tail 1 / one LD iteration / LD loop + remainder / 8 chunks + tail 2 / ... / wide rows
SOME = (12, 64, 300)

# The sizes and spreads below are CONDITIONS on the inputs, found on the CPU and asserted by tests/test_rank_rounding.py: wide enough that
# 60 % of the outputs are untied, narrow enough that every decoy changes five of them.  Short prefixes look at the dense top of a section only,
# so they take more candidates and a narrower spread; long ones need distinct scores further down, so a wider one.
CASES = {}
for _k in WIDTHS:
    CASES["pos_k%d" % _k] = dict(builder="a", k=_k, ncand=500, groups=POS_GROUPS)
for _k in SOME:
    CASES["top10_k%d" % _k] = dict(builder="a", k=_k, ncand=1200, groups=TOP_GROUPS, npos=3, top_k=10, spread=400)
    CASES["top40_k%d" % _k] = dict(builder="a", k=_k, ncand=1200, groups=TOP_GROUPS, npos=3, top_k=40, spread=2500 if _k == 300 else 3000)
    CASES["many_k%d" % _k] = dict(builder="a", k=_k, ncand=500, groups=(8,), npos=many)
    CASES["bans_k%d" % _k] = dict(builder="a", k=_k, ncand=500, groups=POS_GROUPS, nban=25)
    CASES["spec_k%d" % _k] = dict(builder="a", k=_k, ncand=400, groups=(30,), npos=20, spec=True)
for _k in (10, 64, 300):
    CASES["prep_k%d" % _k] = dict(builder="b", k=_k, ncand=500, groups=POS_GROUPS, npos=8)
CASES["top10_bans_k64"] = dict(builder="a", k=64, ncand=1200, groups=TOP_GROUPS, npos=3, top_k=10, nban=25, spread=200, seed=1)
CASES["top10_long_k64"] = dict(builder="a", k=64, ncand=1200, groups=(37, 37), npos=3, top_k=10, spread=200, seed=2)
CASES["sort_k64"] = dict(builder="a", k=64, ncand=2400, groups=(100,), npos=3, top_k=2100, spread=4_000_000)
CASES["group_k16"] = dict(builder="b", k=16, ncand=500, groups=(10, 10, 10, 10), fmt=1)

_built = {}


def case(name):
    if name not in _built:
        _built[name] = Case(**CASES[name])
    return _built[name]


NSEC32_CASES = ("pos_k64", "top10_long_k64")


def main(argv):
    """the child process of test_tiles_of_32_sections_per_wave: the cases of NSEC32_CASES through the GPU ranker with whatever environment the parent
    set, models read from and results written to the directory argv[0]"""
    import os

    import svdfeature_amd as sa
    for name in NSEC32_CASES:
        got, r = case(name).run(lambda f: sa.Ranker(f, 0), os.path.join(argv[0], name + ".model"))
        assert r.counter(3) >= 2, r.counter(3)
        np.save(os.path.join(argv[0], name + ".npy"), got)


if __name__ == "__main__":
    import sys
    main(sys.argv[1:])

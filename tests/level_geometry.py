"""The launch choice of the level kernels of the exact pass -- launch_basicmf, launch_fused, launch_fewrow_fast -- restated in Python from
the comments of svdf_level_geometry.h and the knob table of include/svdfeature_amd.h, and the inputs, configurations and cases of
tests/test_level_geometry.py (CPU: the probe svdf_level_geometry against this rule; the properties of the inputs, proved on numpy level
widths) and tests/test_gpu_level_geometry.py (the HIP engine under every knob combination against the sequential oracle).  Helper module,
not collected.

A level is one conflict-free set of instances, trained by one launch.  Five tuning knobs shape that launch: groups_per_wave (row sets a
wave keeps in flight), block_threads, xcd_remap (grid padded to a multiple of 8, tiles permuted), load_mode and store_mode (cache policy of
the row gathers and stores)."""
import zlib

import numpy as np

import cases
from svdfeature_amd.data import CSRData, pairs_as_csr

F = np.float32
KNOBS = ("groups_per_wave", "block_threads", "xcd_remap", "load_mode", "store_mode")
DEFAULTS = dict(groups_per_wave=0, block_threads=0, xcd_remap=1, load_mode=2, store_mode=0, basic_i8=1, fewrow_i16=1, chain_width=128)
GROUPS = (1, 2, 3, 4, 5, 6, 8)
BLOCKS = (64, 128, 256)
FULL_K = (4, 8, 16, 32, 64, 128, 256)            # k = 4 lanes: one width per lane class
RAGGED_K = (3, 7, 12, 30, 60, 100, 200)          # ... and one that leaves the last lanes of the class partly or wholly empty
WIDTHS = tuple(sorted(FULL_K + RAGGED_K))


# ---------------------------------------------------------------------------------------------------------------- the rule
def lane_class(k):
    """lanes of a lane group: the power of two that holds the row's 16-byte chunks"""
    chunks, lanes = (k + 3) // 4, 1
    while lanes < chunks and lanes < 64:
        lanes *= 2
    return lanes


def load_in_effect(k, load_mode):
    """load_mode 2 = auto: nontemporal for rows of two cache lines (64 floats of pitch) or more"""
    return (1 if (k + 3) // 4 * 4 >= 64 else 0) if load_mode == 2 else load_mode & 1


def auto_groups_k64(n):
    """the eight-lane form at k = 64 aims at ~1 800 waves per launch: one row set up to 21 599 instances, four from 50 400"""
    return min(4, max(1, (n + 7200) // 14400))


def _grid(g, n):
    g["per_set"] = 64 // g["lanes"]
    g["per_block"] = g["block"] // 64 * g["groups"] * g["per_set"]
    g["grid_work"] = -(-n // g["per_block"])
    g["grid"] = (g["grid_work"] + 7) // 8 * 8 if g["remap"] else g["grid_work"]
    return g


def basic_rule(k, n, plain=True, unit=True, **knobs):
    """launch_basicmf for a level of n instances.  plain: the contract configuration (linear link, reg_method 0, user bias, no clamp, no
    per-range decay); unit: every feature value is 1"""
    kn = dict(DEFAULTS, **knobs)
    lanes = lane_class(k)
    slots_cfg = bool(kn["basic_i8"]) and unit and plain
    groups = kn["groups_per_wave"]
    if groups == 0:
        groups = 4 if lanes == 16 else ((1 if slots_cfg and k == 256 else 2) if lanes == 64 else 1)
        if slots_cfg and k == 64:
            groups = auto_groups_k64(n)
    block = kn["block_threads"] or (64 if lanes == 16 else 256)
    fast = plain and kn["store_mode"] == 0
    g = dict(lane_class=lanes, lanes=lanes, chunks=1, full=int(k == 4 * lanes), groups=groups, block=block, nu=0, ni=0, remap=int(bool(kn["xcd_remap"])),
             load=load_in_effect(k, kn["load_mode"]), store=0, knobs=KNOBS, lds=0)
    if unit and fast and k == 64 and kn["basic_i8"]:
        g.update(form="basic_slots8", lanes=8, chunks=2)
    elif unit and fast and k == 256 and kn["basic_i8"]:
        g.update(form="basic_slots16", lanes=16, chunks=4)
    elif unit and fast and g["full"]:
        g.update(form="basic_fast")
    else:
        g.update(form="basic_unit" if unit else "basic_values", store=kn["store_mode"])
    if g["form"].startswith("basic_slots"):            # always nontemporal gathers
        g.update(load=1, knobs=tuple(x for x in KNOBS if x != "load_mode"))
    chain = slots_cfg and kn["store_mode"] == 0 and k == 64
    g.update(chain=int(chain), chain_cap=min(kn["chain_width"], 128) if chain else 0)
    return _grid(g, n)


def fewrow_rule(k, n, nu, ni, fast_cfg=True, has_globals=False, hot=False, **knobs):
    """launch_fused for a level of n instances of at most nu user and ni item ids.  fast_cfg: reg_method 0, no clamp, no per-range decay, no
    relaxed ids -- with a data set free of global features that is the configuration of the few-row fast forms"""
    kn = dict(DEFAULTS, **knobs)
    lanes = lane_class(k)
    block = kn["block_threads"] or 64
    g = dict(lane_class=lanes, lanes=lanes, chunks=1, full=int(k == 4 * lanes), groups=1, block=block, nu=nu, ni=ni, remap=int(bool(kn["xcd_remap"])),
             load=load_in_effect(k, kn["load_mode"]), store=0, lds=0)
    fast = fast_cfg and not has_globals
    if fast and k == 128 and kn["fewrow_i16"]:
        g.update(form="fewrow_slots16", lanes=16, chunks=2, full=1, load=1, knobs=("block_threads", "xcd_remap"))
    elif fast:
        g.update(form="fewrow_fast", knobs=("block_threads", "xcd_remap", "load_mode"))
    elif hot and nu == 2:
        g.update(form="fused_hot", block=1024, knobs=("xcd_remap", "load_mode"))
    elif nu + ni <= 3:
        groups = kn["groups_per_wave"] or (2 if lanes == 16 else 1)
        g.update(form="fused", groups=min(groups, 2), knobs=("groups_per_wave", "block_threads", "xcd_remap", "load_mode"))
    else:
        g.update(form="fused", knobs=("block_threads", "xcd_remap", "load_mode"))
    chain = fast and k == 128 and bool(kn["fewrow_i16"])
    g.update(chain=int(chain), chain_cap=kn["chain_width"] if chain else 0)
    _grid(g, n)
    if g["form"] == "fused_hot":
        g["lds"] = g["per_block"] * (lanes * 16 + 8)
    return g


# ---------------------------------------------------------------------------------------------------------------- configurations
NU, NI, NG = 20000, 16000, 40
# name: (active_type, extra config pairs, plain, fast_cfg).  "contract" is the configuration of the contract workload; the others flip one
# switch of the general instruction stream each
CONFS = {
    "contract": (0, [], True, True),
    "sigmoid": (2, [("base_score", "0.5")], False, True),
    "reg1": (0, [("reg_method", "1"), ("wd_user", "0.02"), ("wd_item", "0.02")], False, False),
    "reg2": (0, [("reg_method", "2"), ("wd_user", "0.5"), ("wd_item", "0.5")], False, False),
    "no_user_bias": (0, [("no_user_bias", "1")], False, True),
    "nonnegative": (0, [("user_nonnegative", "1")], False, False),
    "ranges": (0, [("up:wd", "0.004"), ("up:bound", str(NU // 2)), ("up:wd", "0.02"), ("up:bound", str(NU)),
                   ("ip:wd", "0.001"), ("ip:bound", str(NI // 3)), ("ip:wd", "0.03"), ("ip:bound", str(NI))], False, False),
    "rank": (3, None, False, True),                  # cases.PAIR_CONF: sigmoid rank loss, no user bias
    "rank_reg1": (3, [("reg_method", "1"), ("wd_user", "0.02"), ("wd_item", "0.02")], False, False),
}
SWITCHES = ("sigmoid", "reg1", "reg2", "no_user_bias", "nonnegative", "ranges")


def conf_pairs(name, k, ng=0):
    active, extra, _, _ = CONFS[name]
    if name.startswith("rank"):
        base = cases.conf_with(cases.PAIR_CONF, learning_rate=0.01)
        extra = extra or []
    else:
        base = cases.conf_with(cases.BASICMF_CONF, learning_rate=0.01, wd_user_bias=0.001, wd_item_bias=0.001)
    return cases.conf_with(base, num_user=NU, num_item=NI, num_global=ng, num_factor=k, active_type=active, **({"wd_global": 0.003} if ng else {})) + list(extra)


def setup(t, name, k, ng=0, init=True):
    """the configuration on a trainer (the HIP engine, a host-only probe handle, or the oracle)"""
    t.seed(11)
    for key, v in conf_pairs(name, k, ng):
        t.set_param(key, v)
    if init:
        t.init_model()
        t.init_trainer()
    return t


# ---------------------------------------------------------------------------------------------------------------- inputs
# A level can be no wider than min(users, items), so the inputs have many ids and few ratings each: 24 000 instances over 20 000 x 16 000 ids.
N = 24000
SALT = {"triples": 2, "values": 8, "rows11": 1, "rows22": 3, "rows11g": 3}          # seeds are chosen so that every input's last level is a single instance (tests/test_level_geometry.py asserts it)
_inputs = {}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _ids(rng, n, count, limit):
    """per row `count[r]` distinct ids below limit, as a list of sorted arrays"""
    a = rng.integers(0, limit, (n, 2))
    a[:, 1] = np.where(a[:, 1] == a[:, 0], (a[:, 1] + 1) % limit, a[:, 1])
    return [np.sort(a[r, :count[r]]) for r in range(n)]


def make_input(name):
    """name -> dict(kind, data for the engine and the oracle, ids per row for the level rule, nu, ni, unit, globals).  Labels are 1 .. 5, or
    0 / 1 with `_binary` (sigmoid links)"""
    if name in _inputs:
        return _inputs[name]
    base, _, flag = name.partition("_binary")
    binary = flag != ""
    rng = np.random.default_rng(_seed("level_geometry", base, SALT.get(base, 0)))
    label = rng.integers(0, 2, N).astype(F) if binary else rng.integers(1, 6, N).astype(F)
    d = dict(name=name, nu=1, ni=1, unit=True, has_globals=False, ng=0)
    if base == "triples":            # plain triples: (user, item, rating)
        u, i = rng.integers(0, NU, N).astype(np.uint32), rng.integers(0, NI, N).astype(np.uint32)
        d.update(kind="triples", cols=(u, i, label), csr=CSRData.from_triples(u, i, label), row_ids=np.stack([u.astype(np.int64), NU + i.astype(np.int64)], 1))
    elif base == "values":           # the same structure with feature values other than 1
        u, i = rng.integers(0, NU, N), rng.integers(0, NI, N)
        uv, iv = rng.choice([1.0, 0.5, 0.25, 1.5], N), rng.choice([1.0, -1.0, 0.5, 0.75], N)
        rows = [(float(label[r]), [], [(int(u[r]), float(uv[r]))], [(int(i[r]), float(iv[r]))]) for r in range(N)]
        d.update(kind="rows", csr=CSRData.from_rows(rows), unit=False, row_ids=np.stack([u, NU + i], 1))
    elif base == "pairs":            # rank pairs: one user id, two item ids (positive, negative)
        u, p = rng.integers(0, NU, N), rng.integers(0, NI, N)
        q = (p + 1 + rng.integers(0, NI - 1, N)) % NI
        cols = tuple(x.astype(np.uint32) for x in (u, p, q))
        d.update(kind="pairs", cols=cols, csr=pairs_as_csr(*cols), ni=2, row_ids=np.stack([u, NU + p, NU + q], 1))
    else:                            # rows of up to nu user and ni item ids, some slots absent; `g`: up to three global ids as well
        shape = {"rows11": (1, 1), "rows21": (2, 1), "rows22": (2, 2), "rows11g": (1, 1), "rows12g": (1, 2)}[base]
        ng = NG if base.endswith("g") else 0
        if base == "rows11":         # (all rows 1 + 1 would be plain triples: every seventh row has no user id)
            cu, ci = np.where(np.arange(N) % 7 == 3, 0, 1), np.ones(N, int)
        elif base == "rows11g":
            cu, ci = np.ones(N, int), np.ones(N, int)
        else:
            cu = rng.integers(1, shape[0] + 1, N) if shape[0] == 2 else np.ones(N, int)
            ci = rng.integers(1, shape[1] + 1, N) if shape[1] == 2 else np.ones(N, int)
            cu[::5], ci[::3] = shape[0], shape[1]
        us, its = _ids(rng, N, cu, NU), _ids(rng, N, ci, NI)
        # global ids: few rows carry any, so that levels stay wide (a global id orders all its rows); at most three distinct ones per row
        gs = [np.sort(rng.choice(ng, size=int(rng.integers(1, 4)), replace=False)) if ng and r % 400 == 7 else np.zeros(0, int) for r in range(N)]
        val = lambda: float(rng.choice([1.0, 0.5, -1.0, 0.25]))
        rows = [(float(label[r]), [(int(x), val()) for x in gs[r]], [(int(x), val()) for x in us[r]], [(int(x), val()) for x in its[r]]) for r in range(N)]
        ids = np.full((N, 7), -1, np.int64)
        for r in range(N):
            row = np.concatenate([us[r], NU + its[r], NU + NI + gs[r]])
            ids[r, :len(row)] = row
        d.update(kind="rows", csr=CSRData.from_rows(rows), nu=shape[0], ni=shape[1], unit=False, has_globals=ng > 0, ng=ng, row_ids=ids)
    d["widths"] = level_widths(d["row_ids"], NU + NI + NG)
    _inputs[name] = d
    return d


def level_widths(row_ids, num_ids):
    """widths of the conflict-free levels: an instance's level is one more than the largest last level of its ids (-1: no id)"""
    last = np.zeros(num_ids, np.int64)
    lev = np.zeros(len(row_ids), np.int64)
    for r, row in enumerate(row_ids.tolist()):
        row = [x for x in row if x >= 0]
        l = 1 + max(last[x] for x in row)
        for x in row:
            last[x] = l
        lev[r] = l
    return np.bincount(lev)[1:]


# ---------------------------------------------------------------------------------------------------------------- the GPU cases
class Case:
    """one GPU test function: a launcher, an input, a configuration, a width, knobs that hold for the whole case, and the knob combinations
    looped against one oracle result.  rule(n, combo) is the Python rule for a level of n instances under a combination"""

    def __init__(self, name, launcher, inp, conf, k, base=(), combos=(), kind=None):
        self.name, self.launcher, self.input, self.conf, self.k, self.base, self.combos = name, launcher, inp, conf, k, dict(base), [dict(c) for c in combos]
        self.kind = kind if kind is not None else (0 if launcher == "basic" else 2)
        self.id = "%s-%s-%s-k%d" % (name, inp, conf, k)

    def knobs(self, combo):
        return dict(self.base, **combo)

    def rule(self, n, combo):
        d, (_, _, plain, fast_cfg) = make_input(self.input), CONFS[self.conf]
        kn = {x: v for x, v in self.knobs(combo).items() if x in DEFAULTS}
        if self.launcher == "basic":
            return basic_rule(self.k, n, plain=plain, unit=d["unit"], **kn)
        return fewrow_rule(self.k, n, d["nu"], d["ni"], fast_cfg=fast_cfg, has_globals=d["has_globals"], **kn)

    def probe(self, t, n):
        d = make_input(self.input)
        return t.level_geometry(self.launcher, n, d["nu"], d["ni"], d["unit"], d["has_globals"])


def _sweep(extra=(), groups=GROUPS):
    """every row-set count and every block size at least once (block sizes cycle against the row sets), both remaps, both load policies and,
    with `store`, the two store policies; `extra`: knobs crossed with all of it"""
    out = [dict(groups_per_wave=g, block_threads=BLOCKS[j % 3]) for j, g in enumerate(groups)]
    out += [dict(groups_per_wave=groups[1], block_threads=128, xcd_remap=0), dict(groups_per_wave=groups[-1], block_threads=64, xcd_remap=0)]
    out += [dict(load_mode=0), dict(load_mode=1), dict(groups_per_wave=groups[2], block_threads=128, load_mode=0), dict(groups_per_wave=groups[2], block_threads=128, load_mode=1)]
    return [dict(c, **e) for e in (extra or [{}]) for c in out]


STORES = [dict(store_mode=1), dict(store_mode=2), dict(store_mode=1, groups_per_wave=3, block_threads=128), dict(store_mode=2, groups_per_wave=6, block_threads=256, xcd_remap=0)]
CROSS = [dict(groups_per_wave=g, block_threads=b) for g in GROUPS for b in BLOCKS]
OFF = dict(chain_width=0)          # the level kernel is the subject: no level goes to the chained launch


def _basic_cases():
    out = []
    for j, (kf, kr) in enumerate(zip(FULL_K, RAGGED_K)):
        i8 = [dict(basic_i8=1), dict(basic_i8=0)] if kf in (64, 256) else []
        # the contract configuration: FULL / FAST (the slots forms at 64 and 256; basic_i8 = 0: the lane-group kernel there too) at the full
        # width, the general stream with unit values at the ragged one; store_mode 1 / 2 sends the full width to the general stream as well
        out.append(Case("contract", "basic", "triples", "contract", kf, OFF, _sweep(i8) + STORES))
        out.append(Case("contract", "basic", "triples", "contract", kr, OFF, _sweep() + STORES))
        # one switch of the general stream per width: each of the six at least twice over the fourteen widths
        sf, sr = SWITCHES[j % 6], SWITCHES[(j + 3) % 6]
        out.append(Case("general", "basic", "triples_binary" if sf == "sigmoid" else "triples", sf, kf, OFF, _sweep() + STORES))
        out.append(Case("general", "basic", "triples_binary" if sr == "sigmoid" else "triples", sr, kr, OFF, _sweep() + STORES))
        out.append(Case("values", "basic", "values", "contract", kf, OFF, _sweep() + STORES))
        out.append(Case("values", "basic", "values", "contract", kr, OFF, _sweep() + STORES))
    # row sets x block sizes in full at the three specialised shapes
    out.append(Case("cross_slots8", "basic", "triples", "contract", 64, OFF, CROSS))
    out.append(Case("cross_lanes16", "basic", "triples", "contract", 64, dict(OFF, basic_i8=0), CROSS))
    out.append(Case("cross_slots16", "basic", "triples", "contract", 256, OFF, CROSS))
    # the default chain_width: levels of <= 128 instances go to k_basicmf_slots_chain, the wider ones are launched under non-default knobs
    out.append(Case("chained", "basic", "triples", "contract", 64, {}, [dict(groups_per_wave=3, block_threads=128), dict(groups_per_wave=8, block_threads=256, xcd_remap=0)]))
    return out


FEW_GROUPS = (1, 2, 5)


def _few_sweep(extra=()):
    return _sweep(extra, FEW_GROUPS)


def _fewrow_cases():
    out = []
    fast_inputs = ("pairs", "rows21", "rows22", "rows11")          # the four (NU, NI) shapes: (1, 2), (2, 1), (2, 2), (1, 1)
    for j, k in enumerate(WIDTHS):
        # the few-row fast forms (k_fewrow_fast; k = 128: the sixteen-lane slots form, and with fewrow_i16 = 0 the lane-group kernel)
        inp = fast_inputs[j % 4]
        i16 = [dict(fewrow_i16=1), dict(fewrow_i16=0)] if k == 128 else []
        out.append(Case("fast", "fewrow", inp, "rank" if inp == "pairs" else "contract", k, OFF, _few_sweep(i16)))
        # k_fused: the same shapes under a configuration the fast forms do not take, and rows with global features
        inp = (fast_inputs + ("rows12g", "rows11g"))[(j + 1) % 6]
        conf = "rank_reg1" if inp == "pairs" else (("reg1", "nonnegative", "ranges", "reg2")[j % 4] if not inp.endswith("g") else "contract")
        out.append(Case("fused", "fewrow", inp, conf, k, dict(OFF, fewrow_gslots=0), _few_sweep()))
    for inp in ("rows21", "rows22", "rows11"):                      # the sixteen-lane slots form with every shape (pairs: above)
        out.append(Case("slots16", "fewrow", inp, "contract", 128, OFF, _few_sweep()))
    out.append(Case("fast", "fewrow", "pairs", "rank", 64, OFF, _few_sweep()))   # rank pairs at the width of the benchmark's pair workload's kernel class
    # use_fused = 0: the same rows through the general kernel, which reads none of the five knobs
    out.append(Case("use_fused0", "fewrow", "rows22", "contract", 60, dict(OFF, use_fused=0), _few_sweep()[:7], kind=1))
    # the default chain_width: narrow levels go to k_fewrow_slots_chain
    out.append(Case("chained", "fewrow", "pairs", "rank", 128, {}, [dict(groups_per_wave=5, block_threads=128), dict(groups_per_wave=2, block_threads=256, xcd_remap=0)]))
    return out


BASIC_CASES, FEWROW_CASES = _basic_cases(), _fewrow_cases()
CASES = BASIC_CASES + FEWROW_CASES

"""The launch choice of the level kernels, the parts that need no GPU: the probe svdf_level_geometry -- the functions
launch_basicmf, launch_fused and launch_fewrow_fast call, on a host-only handle -- against the Python statement of the rule in
tests/level_geometry.py; and the properties of the inputs of tests/test_gpu_level_geometry.py, proved on numpy level widths for every
(form, lanes, row sets, block size) that file runs."""
import numpy as np
import pytest

import level_geometry as lg
import svdfeature_amd as sa

# level sizes: 1, both sides of every threshold of the auto rule at k = 64, and (below) one row set +- 1 and one block +- 1 of the case
AUTO_EDGES = (7200, 21600, 36000, 50400, 64800)
SIZES = sorted({1, 2, 3, 100, 24000, 100000} | {e + d for e in AUTO_EDGES for d in (-1, 0, 1)})
KNOB_VALUES = dict(groups_per_wave=(0,) + lg.GROUPS, block_threads=(0,) + lg.BLOCKS, xcd_remap=(0, 1), load_mode=(0, 1, 2), store_mode=(0, 1, 2))


def probe_handle(conf, k, ng=0):
    """the probe needs parameters and knobs only: no model is allocated"""
    active = lg.CONFS[conf][0]
    return lg.setup(sa.Trainer(0, active, 0, device=-2), conf, k, ng, init=False)


def set_knobs(t, knobs):
    for name, v in dict(lg.DEFAULTS, **knobs).items():
        t.set_knob(name, v)


def sizes_of(rule):
    """the level sizes of a cell: the common ones and the edges of its own row set and block"""
    g = rule(1)
    return sorted(set(SIZES) | {max(1, x + d) for x in (g["per_set"], g["per_block"], 8 * g["per_block"], 9 * g["per_block"]) for d in (-1, 0, 1)})


def knob_sets():
    """every value of every knob against the defaults of the others, every row-set count with every block size, and the knobs that reroute"""
    out = [{name: v} for name, vs in KNOB_VALUES.items() for v in vs]
    out += [dict(groups_per_wave=g, block_threads=b, xcd_remap=r) for g in lg.GROUPS for b in lg.BLOCKS for r in (0, 1)]
    out += [dict(store_mode=s, load_mode=m, groups_per_wave=g) for s in (1, 2) for m in (0, 1) for g in (0, 3)]
    return out


@pytest.mark.parametrize("k", lg.WIDTHS)
def test_the_probe_equals_the_rule_basic(k):
    """launch_basicmf: the contract configuration, every switch of the general stream, feature values; every knob value; basic_i8 0 / 1"""
    seen = set()
    for conf in ("contract",) + lg.SWITCHES:
        t = probe_handle(conf, k)
        plain = lg.CONFS[conf][2]
        for unit in (True, False):
            for i8 in (1, 0) if k in (64, 256) else (1,):   # (read at these two widths only)
                for kn in knob_sets():
                    kn = dict(kn, basic_i8=i8)
                    set_knobs(t, kn)
                    rule = lambda n: lg.basic_rule(k, n, plain=plain, unit=unit, **kn)
                    for n in sizes_of(rule):
                        got, want = t.level_geometry("basic", n, unit_values=unit), rule(n)
                        assert got == want, (conf, unit, kn, n, got, want)
                        seen.add((want["form"], want["lanes"], want["groups"]))
        t.close()
    lanes = lg.lane_class(k)
    forms = {f for f, _, _ in seen}
    assert {"basic_unit", "basic_values"} <= forms and ("basic_fast" in forms) == (k == 4 * lanes)
    assert ("basic_slots8" in forms) == (k == 64) and ("basic_slots16" in forms) == (k == 256)
    assert {g for _, _, g in seen} == set(lg.GROUPS)


@pytest.mark.parametrize("k", lg.WIDTHS)
def test_the_probe_equals_the_rule_fewrow(k):
    """launch_fused / launch_fewrow_fast: the four few-row shapes, with and without global features, the configurations the fast forms take
    and those they leave to k_fused; every knob value; fewrow_i16 0 / 1"""
    seen = set()
    for conf in ("contract", "rank", "rank_reg1", "reg1", "reg2", "nonnegative", "ranges", "sigmoid"):
        t = probe_handle(conf, k)
        fast_cfg = lg.CONFS[conf][3]
        for nu, ni in ((1, 1), (1, 2), (2, 1), (2, 2)):
            for glob in (False, True):
                for i16 in (1, 0) if k == 128 else (1,):   # (read at this width only)
                    for kn in knob_sets():
                        kn = dict(kn, fewrow_i16=i16)
                        set_knobs(t, kn)
                        rule = lambda n: lg.fewrow_rule(k, n, nu, ni, fast_cfg=fast_cfg, has_globals=glob, **kn)
                        for n in sizes_of(rule):
                            got, want = t.level_geometry("fewrow", n, nu, ni, False, glob), rule(n)
                            assert got == want, (conf, nu, ni, glob, kn, n, got, want)
                            seen.add((want["form"], want["groups"]))
        t.close()
    assert seen == {("fused", 1), ("fused", 2), ("fewrow_fast", 1)} | ({("fewrow_slots16", 1)} if k == 128 else set())


def test_the_auto_rule_at_k64():
    """the eight-lane form's row sets follow the level size -- min(4, max(1, (n + 7200) / 14400)) -- where no knob asks otherwise; test data
    sets never reach its thresholds, so the probe is the only witness"""
    t = probe_handle("contract", 64)
    set_knobs(t, {})
    want = {7199: 1, 7200: 1, 21599: 1, 21600: 2, 35999: 2, 36000: 3, 50399: 3, 50400: 4, 64800: 4, 10 ** 7: 4, 1: 1}
    for n, groups in want.items():
        g = t.level_geometry("basic", n)
        assert (g["form"], g["lanes"], g["groups"], g["block"]) == ("basic_slots8", 8, groups, 64) and lg.auto_groups_k64(n) == groups, (n, g)
    set_knobs(t, dict(store_mode=1))            # the same count in the general stream (the rule looks at basic_i8, not at the form)
    g = t.level_geometry("basic", 36000)
    assert (g["form"], g["lanes"], g["groups"], g["store"]) == ("basic_unit", 16, 3, 1)
    set_knobs(t, dict(basic_i8=0))              # sixteen lanes: four row sets whatever the size
    assert [t.level_geometry("basic", n)["groups"] for n in (1, 7200, 36000)] == [4, 4, 4]
    t.close()


def test_what_each_knob_reaches():
    """the knob table of svdfeature_amd.h, as the probe reports it: a knob a form ignores changes nothing in its launch"""
    reads = {}
    for k in lg.WIDTHS:
        t = probe_handle("contract", k)
        r = probe_handle("reg1", k)
        for i8 in (0, 1):
            set_knobs(t, dict(basic_i8=i8, fewrow_i16=i8))
            set_knobs(r, dict(basic_i8=i8, fewrow_i16=i8))
            for g in (t.level_geometry("basic", 5000), t.level_geometry("basic", 5000, unit_values=False), r.level_geometry("basic", 5000),
                      t.level_geometry("fewrow", 5000, 1, 2, False), t.level_geometry("fewrow", 5000, 2, 2, False),
                      r.level_geometry("fewrow", 5000, 1, 2, False), r.level_geometry("fewrow", 5000, 2, 2, False), r.level_geometry("fewrow", 5000, 2, 1, False, True)):
                reads.setdefault((g["form"], g["nu"] + g["ni"] == 4), set()).add(g["knobs"])
        t.close()
        r.close()
    all5 = lg.KNOBS
    assert reads == {
        ("basic_fast", False): {all5}, ("basic_unit", False): {all5}, ("basic_values", False): {all5},
        ("basic_slots8", False): {("groups_per_wave", "block_threads", "xcd_remap", "store_mode")},
        ("basic_slots16", False): {("groups_per_wave", "block_threads", "xcd_remap", "store_mode")},
        ("fewrow_fast", False): {("block_threads", "xcd_remap", "load_mode")}, ("fewrow_fast", True): {("block_threads", "xcd_remap", "load_mode")},
        ("fewrow_slots16", False): {("block_threads", "xcd_remap")}, ("fewrow_slots16", True): {("block_threads", "xcd_remap")},
        ("fused", False): {("groups_per_wave", "block_threads", "xcd_remap", "load_mode")}, ("fused", True): {("block_threads", "xcd_remap", "load_mode")},
    }
    # ignored means ignored: the probe's answer does not move with a knob outside `knobs`
    for k, launcher, conf, shape in ((64, "basic", "contract", (1, 1)), (256, "basic", "contract", (1, 1)), (128, "fewrow", "contract", (1, 2)), (100, "fewrow", "contract", (2, 1)),
                                     (60, "fewrow", "reg1", (2, 2)), (60, "fewrow", "reg1", (1, 2))):
        t = probe_handle(conf, k)
        set_knobs(t, {})
        base = t.level_geometry(launcher, 5000, *shape)
        for name, values in KNOB_VALUES.items():
            answers = set()
            for v in values[1:] if name in ("groups_per_wave", "block_threads") else values:
                set_knobs(t, {name: v})
                answers.add(tuple(sorted((a, b) for a, b in t.level_geometry(launcher, 5000, *shape).items())))
            assert (len(answers) > 1) == (name in base["knobs"]), (k, launcher, conf, shape, name)
        t.close()


def test_the_probe_refuses():
    t = probe_handle("contract", 64)
    for args, msg in ((("basic", 0), "bad arguments"), (("fewrow", 10, 3, 1), "few-row shape"), (("fewrow", 10, 1, 0), "few-row shape")):
        with pytest.raises(sa.SvdfError, match=msg):
            t.level_geometry(*args)
    t.set_param("num_factor", "257")
    with pytest.raises(sa.SvdfError, match="num_factor"):
        t.level_geometry("basic", 10)
    t.close()


# ---------------------------------------------------------------------------------------------------------------- the GPU inputs
def test_level_widths_of_the_inputs():
    """the level rule on numpy: many ids and few ratings each give a handful of wide, ragged levels down to a single instance; no row is
    hot (pivot_min 2048) and the data sets stay far below runs_min_rows (2^20), so their kinds are 0 / 1 / 2"""
    for name in sorted({c.input for c in lg.CASES}):
        d = lg.make_input(name)
        w = d["widths"]
        assert w.sum() == lg.N < 1 << 20 and 8 <= len(w) <= 40 and w[0] >= 2048 and w.min() == 1, (name, w.tolist())
        ids = d["row_ids"][d["row_ids"] >= 0]
        assert np.bincount(ids).max() < 2048 // 8
        # a user or an item never meets twice inside a level, and every level follows from the one before: the rule, checked the slow way
    d = lg.make_input("triples")
    u, i = d["cols"][0].astype(np.int64), d["cols"][1].astype(np.int64)
    lu, li, lev = np.zeros(lg.NU, int), np.zeros(lg.NI, int), np.zeros(lg.N, int)
    for r in range(lg.N):
        lev[r] = lu[u[r]] = li[i[r]] = max(lu[u[r]], li[i[r]]) + 1
    assert np.array_equal(np.bincount(lev)[1:], d["widths"])
    for l in range(1, lev.max() + 1):
        assert len(set(u[lev == l])) == len(set(i[lev == l])) == (lev == l).sum()


def _last_wave(n, g):
    """instances of the level's last wave, and how many of its row sets are wholly absent / partly filled"""
    per_wave = g["groups"] * g["per_set"]
    r = n - (n - 1) // per_wave * per_wave
    return r, g["groups"] - -(-r // g["per_set"]), int(r % g["per_set"] != 0)


@pytest.mark.parametrize("case", lg.CASES, ids=[c.id for c in lg.CASES])
def test_the_inputs_reach_the_edges(case):
    """Conditions, not measurements, for every combination a GPU case runs, on the level widths of its input.
      * over the case: a level of at least 9 workgroups with work at the case's smallest tile (the remap permutes real tiles) and one of at
        least 2 at its largest;
      * per combination: a level whose width is no multiple of the instances of a row set; with more than one row set per wave, a level
        whose last wave has a wholly absent row set and a partly filled one; a level narrower than one row set; under the remap, a grid
        with a workgroup without work.
    At 64 lanes per row a row set is ONE instance: it cannot be partly filled, no level is narrower, and every width is a multiple -- there
    the conditions are a wholly absent row set in the last wave and a level of one instance (the narrowest there is)."""
    d = lg.make_input(case.input)
    widths = [int(n) for n in d["widths"]]
    t = probe_handle(case.conf, case.k, d["ng"])
    tiles = []
    for combo in case.combos:
        kn = case.knobs(combo)
        set_knobs(t, {x: v for x, v in kn.items() if x in lg.DEFAULTS})
        shapes = [case.rule(n, combo) for n in widths]
        for n, g in zip(widths, shapes):
            assert case.probe(t, n) == g, (combo, n)
        g = shapes[0]
        if case.kind == 1:                      # the general kernel: the launcher under test is not reached; the GPU case asserts that
            continue
        assert all((s["form"], s["lanes"], s["groups"], s["block"]) == (g["form"], g["lanes"], g["groups"], g["block"]) for s in shapes)
        tiles.append(g["per_block"])
        per_set = g["per_set"]
        last = [_last_wave(n, s) for n, s in zip(widths, shapes)]
        if per_set > 1:
            assert any(n % per_set for n in widths), combo
            assert any(n < per_set for n in widths), combo
            if g["groups"] > 1:
                assert any(absent >= 1 and partly for _, absent, partly in last), (combo, last)
        else:
            assert 1 in widths
            if g["groups"] > 1:
                assert any(absent >= 1 for _, absent, _ in last), (combo, last)
        if g["remap"]:
            assert any(s["grid"] > s["grid_work"] for s in shapes), combo
        assert all(s["grid"] % 8 == 0 for s in shapes) if g["remap"] else all(s["grid"] == s["grid_work"] for s in shapes)
    t.close()
    if tiles:
        assert -(-max(widths) // min(tiles)) >= 9 and -(-max(widths) // max(tiles)) >= 2, (min(tiles), max(tiles), max(widths))


def test_the_cases_cover_what_they_must():
    """every (form, lanes) of launch_basicmf meets every row-set count and every block size, both remaps, both load policies and the two
    store policies; the three specialised shapes meet the full cross; the few-row launchers meet the four shapes, the fold of the row sets,
    the block sizes, the remaps and the load policies at every lane class"""
    basic, few = {}, {}
    for case in lg.CASES:
        if case.kind == 1:
            continue
        for combo in case.combos:
            g = case.rule(5000, combo)
            kn = dict(lg.DEFAULTS, **case.knobs(combo))
            if case.launcher == "basic":
                basic.setdefault((g["form"], g["lanes"], bool(g["full"])), []).append((g["groups"], g["block"], g["remap"], g["load"], g["store"], kn["load_mode"]))
            else:
                few.setdefault((g["form"], g["lanes"]), []).append((g["groups"], g["block"], g["remap"], g["load"], kn["groups_per_wave"], (g["nu"], g["ni"]), kn["load_mode"]))
    lanes7 = (1, 2, 4, 8, 16, 32, 64)
    want = {("basic_fast", l, True) for l in lanes7} | {("basic_slots8", 8, True), ("basic_slots16", 16, True)}
    want |= {(f, l, full) for f in ("basic_unit", "basic_values") for l in lanes7 for full in (True, False)}
    assert set(basic) == want
    for key, seen in basic.items():
        assert {s[0] for s in seen} == set(lg.GROUPS) and {s[1] for s in seen} == set(lg.BLOCKS) and {s[2] for s in seen} == {0, 1}, key
        assert {s[5] for s in seen} >= {0, 1}, key                       # load_mode 0 and 1 set ...
        assert {s[3] for s in seen} == ({1} if key[0].startswith("basic_slots") else {0, 1}), key   # ... and in effect where the form reads it
        assert {s[4] for s in seen} == ({0, 1, 2} if key[0] in ("basic_unit", "basic_values") else {0}), key
    for key in (("basic_slots8", 8, True), ("basic_fast", 16, True), ("basic_slots16", 16, True)):
        assert {(s[0], s[1]) for s in basic[key]} == {(g, b) for g in lg.GROUPS for b in lg.BLOCKS}, key
    assert set(few) == {(f, l) for f in ("fewrow_fast", "fused") for l in lanes7} | {("fewrow_slots16", 16)}
    for key, seen in few.items():
        assert {s[1] for s in seen} == set(lg.BLOCKS) and {s[2] for s in seen} == {0, 1} and {s[4] for s in seen} >= {1, 2, 5} and {s[6] for s in seen} >= {0, 1}, key
        assert {s[3] for s in seen} == ({1} if key[0] == "fewrow_slots16" else {0, 1}), key
        # the fold: above two row sets k_fused takes two, with 2 + 2 id slots one; the fast forms always one
        for groups, _, _, _, asked, shape, _ in seen:
            asked = asked or (2 if key[1] == 16 else 1)                  # 0 = auto: two row sets at 16 lanes per row
            assert groups == (1 if key[0] != "fused" or sum(shape) == 4 else min(asked, 2)), (key, asked, shape)
    for form in ("fewrow_fast", "fused", "fewrow_slots16"):
        assert {s[5] for key, seen in few.items() if key[0] == form for s in seen} == {(1, 1), (1, 2), (2, 1), (2, 2)}, form
    assert any(c.conf == "rank" and c.input == "pairs" for c in lg.CASES)
    assert {c.conf for c in lg.BASIC_CASES if c.name == "general"} == set(lg.SWITCHES)

"""The launch geometry of the live-model ranking calls stated in Python, and the inputs of the sweeps over it (helper of
tests/test_rank_geometry.py and tests/test_gpu_rank_geometry.py; not collected).

The rule.  An item TILE is what one pass of a sweep scores: 128 items for rows of up to 128 floats (two candidates per lane), 64 for wider
rows.  The items are split over gy RANGES of whole tiles, one workgroup (wide top-N sweep: one wave) in y each: as many ranges as give
about 2048 workgroups (wide top-N: 8192 waves) over the call's units -- tiles of 64 sections or rows; wide top-N: sections -- but at
least 8 item tiles per range where the items allow, for top-N at most `rank_topn_budget / capacity` lists per piece, and at most 65535.
The ranges are equal, ceil(tiles / split) tiles each, so the last one may be ragged or as short as one item, and gy may come out below
the split.  The wide evaluation sweep has no ranges (every item lies in grid.x) but takes one launch per 32768 rows.  A top-N list has
room for top_n kept keys plus one tile of appends, twice top_n where 512 keys -- one wave's sort buffer -- allow."""
import numpy as np

F32 = np.float32
TILE_SECTIONS = 64        # sections (rows) of one workgroup of a narrow sweep
TILE_POSITIVES = 512      # thresholds of one evaluation tile, and the most positives of one row
SORT_KEYS = 512           # keys one wave sorts in LDS: the largest list capacity
WIDE_ROWS = 32768         # rows of one launch of the wide evaluation sweep
EVAL_BUDGET, TOPN_BUDGET = 1 << 22, 1 << 25   # the knobs' defaults


def pitch_of(k):
    return (k + 3) // 4 * 4


def item_tile(k):
    return 128 if pitch_of(k) <= 128 else 64


def wide(k):
    return pitch_of(k) > 256


def _split(num_item, ti, units, want, most=65535):
    ntile = -(-num_item // ti)
    ysplit = max(1, min(-(-want // max(1, units)), (ntile + 7) // 8))
    ysplit = min(ysplit, most, 65535)
    per = -(-ntile // ysplit) * ti
    return -(-num_item // per), per


def topn_cap(k, top_n):
    ti = item_tile(k)
    cap = 128
    while cap < 2 * top_n + ti:
        cap *= 2
    return min(max(cap, top_n + ti), SORT_KEYS)


def cap_regime(k, top_n):
    """which arm of the capacity rule decides: "start" (128 without doubling), "doubled", "ceiling" (the doubling passed 512)"""
    need = 2 * top_n + item_tile(k)
    return "start" if need <= 128 else ("doubled" if need <= SORT_KEYS else "ceiling")


def topn_geometry(k, num_item, nsec, top_n, budget=TOPN_BUDGET):
    """what svdf_rank_geometry answers for kind "topn": the first piece of nsec sections without bans"""
    cap = topn_cap(k, top_n)
    max_lists = max(1, budget // cap)
    piece = min(nsec, max_lists)
    if piece > 64 and piece < nsec:
        piece -= piece % 64
    ts = 1 if wide(k) else TILE_SECTIONS
    units = -(-piece // ts)
    gy, per = _split(num_item, item_tile(k), units, 8192 if wide(k) else 2048, max(1, max_lists // max(1, piece)))
    return dict(gy=gy, items_per_block=per, cap=cap, tile_rows=ts, rows=piece, tiles=units, sections=piece, launches=1)


def eval_rows(pos_ptr, tile_rows):
    """(rows, tiles) of sections with the positives pos_ptr: a row is a section or a slice of 512 of its positives; a tile holds up to
    tile_rows consecutive rows and up to 512 positives"""
    n = np.diff(np.asarray(pos_ptr, np.int64))
    per_row = np.concatenate([[TILE_POSITIVES] * (x // TILE_POSITIVES) + ([x % TILE_POSITIVES] if x % TILE_POSITIVES else []) for x in n.tolist()] or [[]]).astype(np.int64)
    tiles, r = 0, 0
    while r < len(per_row):
        e, held = r + 1, per_row[r]
        while e < len(per_row) and e - r < tile_rows and held + per_row[e] <= TILE_POSITIVES:
            held += per_row[e]
            e += 1
        tiles, r = tiles + 1, e
    return len(per_row), tiles


def eval_geometry(k, num_item, tiles=None, pos_ptr=None, budget=EVAL_BUDGET):
    """what svdf_rank_geometry answers for kind "positions": for `tiles` row tiles, or for the first piece of the sections of pos_ptr"""
    ts = 1 if wide(k) else TILE_SECTIONS
    rows = piece = 0
    if pos_ptr is not None:
        load = np.cumsum(np.diff(np.asarray(pos_ptr, np.int64)) + 1)
        piece = max(1, int(np.searchsorted(load, budget, side="right")))
        rows, tiles = eval_rows(pos_ptr[:piece + 1], ts)
    if wide(k):
        gy, per, launches = (1, num_item, -(-rows // WIDE_ROWS)) if tiles else (0, 0, 0)
    else:
        gy, per = _split(num_item, item_tile(k), tiles, 2048) if tiles else (0, 0)
        launches = 1 if tiles else 0
    return dict(gy=gy, items_per_block=per, cap=0, tile_rows=ts, rows=rows, tiles=tiles, sections=piece, launches=launches)


def item_count(k, nsec, gy, last, top_n=1):
    """the smallest catalogue that rank_topn splits, for nsec sections of width k, into gy ranges the last of which holds `last` items
    ("full": as many as the others)"""
    for n in range(1, 1 << 18):
        g = topn_geometry(k, n, nsec, top_n)
        if g["gy"] == gy and n - (gy - 1) * g["items_per_block"] == (g["items_per_block"] if last == "full" else last):
            return n
    raise ValueError("no item count gives gy = %d with a last range of %s" % (gy, last))


def range_of(item, per):
    return np.asarray(item) // per


# ---- the geometries of tests/test_gpu_rank_geometry.py: (num_factor, items, gy, width of the last range); 70 sections -- a full section
# tile and a ragged one.  tests/test_rank_geometry.py asserts each through the probe.
NS, NU = 70, 30
GEOMETRIES = {
    "two-per-lane-gy3": (8, 2177, 3, 641),
    "two-per-lane-gy7-full": (64, 6272, 7, 896),
    "two-per-lane-gy8-one": (8, 7169, 8, 1),
    "two-per-lane-gy14": (8, 14000, 14, 688),
    "one-per-lane-gy8-one": (200, 3585, 8, 1),
    "wide-gy8-one": (260, 3585, 8, 1),
}
CUT_GEOMETRIES = ("two-per-lane-gy3", "one-per-lane-gy8-one", "wide-gy8-one")
CUT_TOPS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
MODELS = ("increasing", "decreasing", "equal", "ties", "winners", "boundary")


def ptr_of(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)


def winners_of(ni, per, gy, seed=0):
    """one id per range: the last id of the first range, the last item of the catalogue, a random id of every range between"""
    rng = np.random.default_rng(seed)
    w = [int(rng.integers(y * per, min((y + 1) * per, ni))) for y in range(gy)]
    w[0], w[-1] = per - 1, ni - 1
    return np.array(w, np.int64)


def boundary_pairs(ni, per, gy):
    """(last id of range y, first id of range y + 1) for every y"""
    return [((y + 1) * per - 1, (y + 1) * per) for y in range(gy - 1)]


def geometry_model(case, nu, ni, k, per, gy):
    """integer-valued models on which every score is exact in fp32 in any order.  "winners": scores within +-(k - 1) but for one planted
    score of about 1000 + y in every range y.  "boundary": every other score negative; the two ids on either side of the boundary behind
    range y score 500 + y both -- boundary 0: -0 on the last id of range 0 and +0 on the first id of range 1 (zero rows, biases -0 / +0)"""
    rng = np.random.default_rng(len(case) + k)
    U = rng.integers(-1, 2, (nu, k)).astype(F32)
    W = rng.integers(-1, 2, (ni, k)).astype(F32)
    bias = np.zeros(ni, F32)
    U[:, 0] = 1.0
    W[:, 0] = 0.0
    if case == "winners":
        for y, w in enumerate(winners_of(ni, per, gy)):
            W[w, 0] = 1000.0 + y
    else:
        bias[:] = -(k + 5.0 + np.arange(ni) % 7)
        for y, (a, b) in enumerate(boundary_pairs(ni, per, gy)):
            W[[a, b]] = 0.0
            bias[[a, b]] = 0.0
            W[[a, b], 0] = 500.0 + y if y else 0.0
        a, b = boundary_pairs(ni, per, gy)[0]
        bias[a], bias[b] = F32(-0.0), F32(0.0)
    return U, W, bias


def exact_scores(U, W, bias):
    """the [user][item] scores of an integer-valued model: the float64 product narrowed to fp32, and whether the narrowing was exact"""
    s64 = bias.astype(np.float64)[None, :] + U.astype(np.float64) @ W.astype(np.float64).T
    s32 = s64.astype(F32)
    return s32, bool(np.array_equal(s32.astype(np.float64), s64))


EMPTY_MIDDLE, EMPTY_FIRST, FEW_LEFT, LEFT = 3, 4, 5, 40   # sections of geometry_bans, and how many items FEW_LEFT leaves


def geometry_bans(S, nu, ni, per, gy, seed):
    """users and ban lists: 0 - 40 banned ids with duplicate entries; section EMPTY_MIDDLE bans the whole range gy // 2, EMPTY_FIRST the whole
    first range, FEW_LEFT all but LEFT items spread over the ranges (one of them the last item)"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    ban = []
    for s in range(S):
        b = rng.permutation(ni)[:int(rng.integers(0, 41))]
        if s == EMPTY_MIDDLE:
            m = gy // 2
            b = np.concatenate([b, np.arange(m * per, min((m + 1) * per, ni))])
        elif s == EMPTY_FIRST:
            b = np.arange(per)
        elif s == FEW_LEFT:
            keep = np.unique(np.concatenate([[ni - 1], np.linspace(0, ni - 1, LEFT).astype(np.int64)]))
            keep = np.unique(np.concatenate([keep, np.setdiff1d(np.arange(ni), keep)[:LEFT - len(keep)]]))
            b = np.setdiff1d(np.arange(ni), keep)
        if len(b) > 1:
            b = np.concatenate([b, b[:int(rng.integers(1, 4))]])
            b = b[rng.permutation(len(b))]
        ban.append(b.astype(np.uint32))
    return users, ptr_of(ban), np.concatenate(ban)


BIG, TIE_SECTION, NPOS_BIG = 10, 11, 600


def geometry_positives(S, ni, per, gy, ban_ptr, ban_item, seed):
    """positives that are not banned: one in every range and up to three more per section; section BIG has 600 (more than one threshold
    tile); section TIE_SECTION holds both ids of every range boundary (they tie under the "boundary" model)"""
    rng = np.random.default_rng(seed)
    pos = []
    for s in range(S):
        free = np.setdiff1d(np.arange(ni), ban_item[ban_ptr[s]:ban_ptr[s + 1]])
        ys = range_of(free, per)
        each = np.array([rng.choice(free[ys == y]) for y in np.unique(ys)])
        if s == BIG:
            p = np.concatenate([each, rng.permutation(np.setdiff1d(free, each))[:NPOS_BIG - len(each)]])
        elif s == TIE_SECTION:
            p = np.intersect1d(np.array(boundary_pairs(ni, per, gy)).ravel(), free)
        else:
            p = np.unique(np.concatenate([each, rng.choice(free, 3)]))
        p = p[rng.permutation(len(p))]
        pos.append(p.astype(np.uint32))
    return ptr_of(pos), np.concatenate(pos)


_inputs = {}


def geometry_inputs(name):
    """the shapes, sections and lists of one of GEOMETRIES, built once and shared (nothing changes them)"""
    if name not in _inputs:
        k, ni, gy, last = GEOMETRIES[name]
        g = topn_geometry(k, ni, NS, 1)
        per = g["items_per_block"]
        users, ban_ptr, ban_item = geometry_bans(NS, NU, ni, per, gy, seed=gy + k)
        pos_ptr, pos_item = geometry_positives(NS, ni, per, gy, ban_ptr, ban_item, seed=gy + k + 1)
        _inputs[name] = dict(name=name, k=k, ni=ni, gy=gy, last=last, per=per, users=users, ban_ptr=ban_ptr, ban_item=ban_item, pos_ptr=pos_ptr,
                             pos_item=pos_item)
    return _inputs[name]


def model_for(case, c):
    """(U, W, bias) of one of MODELS on the shapes of c = geometry_inputs(..); the four pressure models are test_gpu_rank_topn.pressure_model's"""
    if case in ("winners", "boundary"):
        return geometry_model(case, NU, c["ni"], c["k"], c["per"], c["gy"])
    from test_gpu_rank_topn import pressure_model
    return pressure_model(case, NU, c["ni"], c["k"], np.random.default_rng(len(case)))


def cut_lists(want, top_n):
    """rule_topn's tuple for a shorter list, from the one for a longer: the rule sorts a section once and keeps a prefix"""
    items, scores, count, nan = want
    return items[:, :top_n].copy(), scores[:, :top_n].copy(), np.minimum(count, top_n).astype(np.int32), nan.copy()


def only_first_ranges(ban_ptr, ban_item, ni, per, ranges=2):
    """the decoy of a merge that reads only the first `ranges` lists of a section: ban lists that also ban every id behind them"""
    out = [np.concatenate([ban_item[a:b], np.arange(min(ranges * per, ni), ni, dtype=np.uint32)]) for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    return ptr_of(out), np.concatenate(out)


# ---- the row chunks of the wide evaluation sweep: num_factor 260; 32768 + 40 rows; the sections FIRST_BIG and STRADDLE have 600 positives,
# so two rows each -- rows 0 / 1 and rows 32767 / 32768, the last row of the first launch and the first row of the second; every other
# section has one positive.  BEHIND is the section of row 32769: in the second launch it has the place that row 1, no first row, has in the first.
CH_K, CH_NI, CH_NU = 260, 641, 50
CH_ROWS = WIDE_ROWS + 40
FIRST_BIG, STRADDLE, BEHIND = 0, WIDE_ROWS - 2, WIDE_ROWS - 1
CH_S = CH_ROWS - 2
NAN_ITEM = CH_NI - 1


def chunk_model():
    rng = np.random.default_rng(260)
    return rng.integers(-1, 2, (CH_NU, CH_K)).astype(F32), rng.integers(-1, 2, (CH_NI, CH_K)).astype(F32), rng.integers(-2, 3, CH_NI).astype(F32)


def chunk_sections(nan_call=False):
    """(users, pos_ptr, pos_item, ban_ptr, ban_item); no positive is NAN_ITEM.  nan_call: every section but STRADDLE and BEHIND bans NAN_ITEM"""
    rng = np.random.default_rng(7)
    users = rng.integers(0, CH_NU, CH_S).astype(np.uint32)
    npos = np.ones(CH_S, np.int64)
    npos[[FIRST_BIG, STRADDLE]] = NPOS_BIG
    pos_ptr = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    pos_item = rng.integers(0, CH_NI - 1, int(pos_ptr[-1])).astype(np.uint32)
    for s in (FIRST_BIG, STRADDLE):
        pos_item[pos_ptr[s]:pos_ptr[s + 1]] = rng.permutation(CH_NI - 1)[:NPOS_BIG]
    own = pos_item[pos_ptr[:-1]]
    other = ((own + 1 + rng.integers(0, CH_NI - 3, CH_S)) % (CH_NI - 1)).astype(np.uint32)   # one banned id per section, never its positive
    ban = [[] if s in (FIRST_BIG, STRADDLE) else [other[s]] for s in range(CH_S)]
    if nan_call:
        ban = [b if s in (STRADDLE, BEHIND) else b + [NAN_ITEM] for s, b in enumerate(ban)]
    return users, pos_ptr, pos_item, ptr_of(ban), np.array([x for b in ban for x in b], np.uint32)


def rule_positions_rows(scores, users, pos_ptr, pos_item, ban_ptr, ban_item):
    """the documented rule (tests/test_gpu_rank_eval.py: rule_positions) for many sections at once: scores is [user][item]; returns
    (position, tied, ranked, nan) as Trainer.rank_positions does"""
    S, ni = len(users), scores.shape[1]
    on = np.ones((S, ni), bool)
    on[np.repeat(np.arange(S), np.diff(ban_ptr)), ban_item.astype(np.int64)] = False
    sec = np.repeat(np.arange(S), np.diff(pos_ptr))
    p = pos_item.astype(np.int64)
    position, tied = np.zeros(len(p), np.int32), np.zeros(len(p), np.int32)
    ids = np.arange(ni)
    for a in range(0, len(p), 4096):
        q = slice(a, a + 4096)
        row = scores[users[sec[q]].astype(np.int64)]
        thr = row[np.arange(len(p[q])), p[q]][:, None]
        live = on[sec[q]]
        eq = live & (row == thr) & (ids[None, :] != p[q][:, None])
        position[q] = (live & (row > thr)).sum(1) + (eq & (ids[None, :] < p[q][:, None])).sum(1)
        tied[q] = eq.sum(1)
    nan = (on & np.isnan(scores[users.astype(np.int64)])).any(1).astype(np.int32)
    bad = nan[sec] != 0
    position[bad], tied[bad] = -1, -1
    return position, tied, on.sum(1).astype(np.int32), nan

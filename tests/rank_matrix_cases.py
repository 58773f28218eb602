"""The launch geometries of the top-N sweep on the matrix cores (knob rank_topn_scores = 1), the inputs of the tests over them
and the decoys those inputs must tell from the rule (helper of tests/test_rank_matrix_cases.py and tests/test_gpu_rank_matrix_geometry.py;
not collected).

The matrix rule is the pinned rule of rows of up to 128 floats at EVERY width (tests/test_rank_matrix.py: matrix_geometry): tiles of 128
items, 64 sections per workgroup, room for top_n kept keys plus 128 appends.  So everything here calls tests/rank_geometry.py with
min(k, 128); the ban lists, the integer models, the winners and the boundary pairs are that module's, on the matrix sweep's range width."""
import numpy as np

import rank_geometry as rg
from test_gpu_rank_matrix import allowed, plain_topn

F32 = np.float32
TILE = 128                # items of one tile of the matrix sweep, at every width
NS, NU = rg.NS, rg.NU


def mk(k):
    """the width the pinned rule is asked for"""
    return min(k, 128)


def matrix_cap(k, top_n):
    return rg.topn_cap(mk(k), top_n)


# (num_factor, items, gy, width of the last range); 70 sections.  The smallest catalogues with each shape, where "ragged" is a last range
# narrower than the others that ends in a tile of 65 items -- more than one 64-bit ban-mask word, fewer than two: 2 113 = 2 x 768 + 4 x 128 +
# 65 and 13 505 = 13 x 1 024 + 128 + 65.  k = 33: two K chunks, the second a tail of one float; 200: the pinned tile would be 64 items;
# 260: the pinned route is the wide sweep (under the pinned rule 3 585 items give these widths gy = 8, under the matrix rule gy = 4).
GEOMETRIES = {
    "k8-gy3-ragged": (8, 2113, 3, 577),
    "k64-gy7-full": (64, 6272, 7, 896),
    "k33-gy8-one": (33, 7169, 8, 1),
    "k200-gy8-one": (200, 7169, 8, 1),
    "k260-gy8-one": (260, 7169, 8, 1),
    "k1024-gy3-ragged": (1024, 2113, 3, 577),
    "k8-gy14-ragged": (8, 13505, 14, 193),
}
NAMES = tuple(GEOMETRIES)
CUT_GEOMETRIES = ("k8-gy3-ragged", "k200-gy8-one", "k260-gy8-one")
ONE_ITEM_LAST = tuple(n for n in NAMES if GEOMETRIES[n][3] == 1)
TOPS = (1, 100, 256)


def tops_of(case, gy):
    return TOPS + ((gy, gy + 1) if case == "winners" else ())


_inputs, _want = {}, {}


def inputs(name):
    """the shapes, users and ban lists of one of GEOMETRIES under the matrix rule, built once and shared (nothing changes them)"""
    if name not in _inputs:
        k, ni, gy, last = GEOMETRIES[name]
        per = rg.topn_geometry(mk(k), ni, NS, 1)["items_per_block"]
        users, ban_ptr, ban_item = rg.geometry_bans(NS, NU, ni, per, gy, seed=gy + k)
        _inputs[name] = dict(name=name, k=k, ni=ni, gy=gy, last=last, per=per, users=users, ban_ptr=ban_ptr, ban_item=ban_item)
    return _inputs[name]


def tail_start(c):
    """the first id of the ragged last tile of the last range; ni where the last tile is whole"""
    return c["ni"] - c["ni"] % TILE


def int_scores(U, W, bias, users):
    """the [section][item] scores of an integer-valued model in int64: exact, and a zero is +0"""
    return bias.astype(np.int64)[None, :] + U[users].astype(np.int64) @ W.astype(np.int64).T


def want_lists(name, case):
    """(plain_topn at top_n = 256 -- shorter lists are its prefixes, rg.cut_lists --, the int64 scores, the model) of one geometry's lists
    under one of rg.MODELS; computed once and shared"""
    if (name, case) not in _want:
        c = inputs(name)
        U, W, bias = rg.model_for(case, c)
        score = int_scores(U, W, bias, c["users"])
        _want[(name, case)] = plain_topn(score, allowed(NS, c["ni"], c["ban_ptr"], c["ban_item"]), 256), score, (U, W, bias)
    return _want[(name, case)]


def holds_zero(lists):
    """per section: whether a listed score is zero"""
    items, scores, count, _ = lists
    return np.array([(scores[s, :count[s]] == 0).any() for s in range(len(count))])


def float_model(nu, ni, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nu, k)).astype(F32), rng.standard_normal((ni, k)).astype(F32), rng.standard_normal(ni).astype(F32)


# ---- the decoys: what a wrong sweep or merge would list, stated on the int64 scores
DECOYS = ("bans-behind-range-0", "tail-tile-dropped", "two-lists-merged", "larger-id-first", "append-order")


def decoy_lists(decoy, c, score, top_n):
    """bans-behind-range-0: a ban cursor that never advances past range 0 -- the bans of the ranges y > 0 are ignored;
    tail-tile-dropped: the ragged last tile of the last range is not ranked;
    two-lists-merged: rg.only_first_ranges, a merge that reads two lists;
    larger-id-first: equal scores by the LARGER id;
    append-order: a cut that keeps the keys in append order -- top_n taken from the first `cap` unbanned ids of every range"""
    ni, per = c["ni"], c["per"]
    ids = np.arange(ni)
    on = allowed(NS, ni, c["ban_ptr"], c["ban_item"])
    if decoy == "bans-behind-range-0":
        on = on | (ids >= per)[None, :]
    elif decoy == "tail-tile-dropped":
        on = on & (ids < tail_start(c))[None, :]
    elif decoy == "two-lists-merged":
        on = allowed(NS, ni, *rg.only_first_ranges(c["ban_ptr"], c["ban_item"], ni, per))
    elif decoy == "larger-id-first":
        items, scores, count, nan = plain_topn(score[:, ::-1], on[:, ::-1], top_n)       # the smaller mirrored id is the larger id
        return np.where(items >= 0, ni - 1 - items, -1).astype(np.int32), scores, count, nan
    elif decoy == "append-order":
        seen = np.cumsum(on, axis=1)
        first = np.repeat(np.concatenate([np.zeros((NS, 1), seen.dtype), seen[:, per - 1::per]], axis=1)[:, :c["gy"]], per, axis=1)[:, :ni]
        on = on & (seen - first <= matrix_cap(c["k"], top_n))
    else:
        raise ValueError(decoy)
    return plain_topn(score, on, top_n)


def blind(name, case, decoy):
    """the (geometry, model) pairs that cannot see a decoy, and why"""
    if decoy == "tail-tile-dropped":
        return GEOMETRIES[name][1] % TILE == 0                  # the last tile is whole: nothing to drop
    if decoy == "larger-id-first":
        return case in ("increasing", "decreasing")             # scores strictly monotone in the id: nothing ties
    if decoy == "append-order":
        return case in ("decreasing", "equal")                  # the best keys of a range ARE its first unbanned ids
    return False                                                # section FEW_LEFT bans and keeps ids of every range: both ban decoys show


# ---- how often the sweep cuts a list
def forced_cuts(appends, cap, top_n):
    """the cuts of one list over the tiles of a range, every candidate beating the threshold: appends[t] keys into `cap` slots, cut to
    top_n when cnt + 128 > cap"""
    cnt = cuts = 0
    for a in appends:
        if cnt + TILE > cap:
            cnt, cuts = min(cnt, top_n), cuts + 1
        cnt += a
        assert cnt <= cap
    return cuts


def tile_appends(c, s, y):
    """the unbanned items of every tile of range y for section s"""
    on = np.ones(c["ni"], bool)
    on[c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]].astype(np.int64)] = False
    r = on[y * c["per"]:min((y + 1) * c["per"], c["ni"])]
    return [int(r[a:a + TILE].sum()) for a in range(0, len(r), TILE)]


# ---- scores do not depend on where they are computed
GRID_KS = (7, 64, 130, 320)
GRID_SMALL, GRID_LARGE = 517, 2113          # gy = 1 and gy = 3 at every width; 2 113 - 517 = 12 x 128 + 60: the moved rows sit elsewhere in their tiles
SAME_USER, SAME_AT = 5, (0, 17, 37, 64)     # one user at four lane-group / wave / tile positions of the section tiles


def grid_bans(seed):
    """ban lists over the ids 0 .. 516, 0 - 40 per section with duplicates (rg.geometry_bans on one range)"""
    return rg.geometry_bans(NS, NU, GRID_SMALL, GRID_SMALL, 1, seed)


def shifted_bans(ban_ptr, ban_item, shift, lo, hi):
    """the same lists with their ids moved by `shift`, every section also banning lo .. hi - 1"""
    out = [np.concatenate([ban_item[a:b] + np.uint32(shift), np.arange(lo, hi, dtype=np.uint32)]) for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    return rg.ptr_of(out), np.concatenate(out)


def planted_ids(c):
    """where the copies of one item row go on a geometry with a ragged last range: the first id; tile position 16 b + 15 for b = 2 in the
    first tile of range 1 and b = 5 in the second tile of the last range; the first id of the ragged last tile; the last item"""
    per, gy = c["per"], c["gy"]
    ids = [0, per + 16 * 2 + 15, (gy - 1) * per + TILE + 16 * 5 + 15, tail_start(c), c["ni"] - 1]
    assert len(set(ids)) == 5 and ids == sorted(ids) and ids[2] < ids[3]
    return np.array(ids, np.int64)


def planted_sections(c):
    """(users, ban_ptr, ban_item, kept): section s keeps the copy kept[s] and bans the four others, besides its own bans; SAME_USER sits at
    SAME_AT with four different copies"""
    copies = planted_ids(c)
    users = c["users"].copy()
    users[list(SAME_AT)] = SAME_USER
    kept = np.arange(NS) % 5
    kept[list(SAME_AT)] = [0, 1, 2, 3]
    ban = []
    for s in range(NS):
        b = c["ban_item"][c["ban_ptr"][s]:c["ban_ptr"][s + 1]].astype(np.int64)
        if s in (rg.EMPTY_MIDDLE, rg.EMPTY_FIRST, rg.FEW_LEFT):
            b = b[:7]                                            # (these three sections ban whole ranges: here they are ordinary)
        b = np.concatenate([b[~np.isin(b, copies)], np.delete(copies, kept[s])])
        ban.append(b.astype(np.uint32))
    return users, rg.ptr_of(ban), np.concatenate(ban), copies[kept]

"""Batch ranking evaluation on the live model (svdf_rank_eval_*, svdf_k_rankeval.hip) on the GPU.  The checker is the pinned
port's ranker, oracle.OracleRanker("port", 0, 0), fed the same sections as tag lines from the model saved to a temporary file, the way
tests/test_gpu_ranker.py does it; ties, where the port's order is its sort's, are checked against an integer numpy statement of the rule."""
import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from rank_rounding import score_fp32
from test_rank_eval import auc_restated

pytestmark = pytest.mark.gpu
F32 = np.float32


def new_trainer(nu, ni, k, seed=3, conf=cases.BASICMF_CONF, active=0, extra=()):
    t = sa.Trainer(0, active)
    t.seed(seed)
    for kk, v in cases.conf_with(conf, num_user=nu, num_item=ni, num_factor=k, ui_init_sigma=0.1) + list(extra):
        t.set_param(kk, v)
    t.init_model()
    t.init_trainer()
    return t


def make_sections(S, nu, ni, seed, big=10, empty=20, full_ban=30, npos_big=300):
    """S sections: 1 - 5 positives each, section `big` with npos_big, section `empty` with none; 0 - 40 banned items with duplicate entries;
    section `full_ban` bans everything but its positives; user 7 in three sections"""
    rng = np.random.default_rng(seed)
    users = rng.integers(0, nu, S).astype(np.uint32)
    users[[0, S // 4, S // 2]] = 7
    pos, ban = [], []
    for s in range(S):
        npos = npos_big if s == big else (0 if s == empty else int(rng.integers(1, 6)))
        perm = rng.permutation(ni)
        p = perm[:npos]
        rest = perm[npos:]
        b = rest if s == full_ban else rest[:int(rng.integers(0, 41))]
        if len(b) > 1:
            b = np.concatenate([b, b[:int(rng.integers(1, 4))]])   # duplicate ban entries count once
            b = b[rng.permutation(len(b))]
        pos.append(p.astype(np.uint32))
        ban.append(b.astype(np.uint32))
    ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    return users, ptr(pos), np.concatenate(pos), ptr(ban), np.concatenate(ban)


def port_positions(path, ni, users, pos_ptr, pos_item, ban_ptr, ban_item):
    """the same sections through the port's ranker: candidates are the ITEM lines i:1 for every item id (index == id); a section is a USER
    line, a POS_SAMPLE line, a BAN_SAMPLE line of its DISTINCT banned ids and a PROCESS line"""
    r = oracle.OracleRanker("port", 0, 0)
    r.set_param("top_k", "0")
    r.load_model(path)
    r.init_ranker(ni)
    r.process_rows(sa.CSRData.from_rows([(0.0, [], [], [(c, 1.0)]) for c in range(ni)]))
    out = []
    for s in range(len(users)):
        p = pos_item[pos_ptr[s]:pos_ptr[s + 1]]
        if len(p) == 0:
            continue
        rows = [(2.0, [], [(int(users[s]), 1.0)], []), (1.0, [], [(int(x), 1.0) for x in p], [])]
        b = ban_item[ban_ptr[s]:ban_ptr[s + 1]] if ban_ptr is not None else []
        if len(b):
            _, first = np.unique(b, return_index=True)
            rows.append((-1.0, [], [(int(x), 1.0) for x in np.asarray(b)[np.sort(first)]], []))
        rows.append((4.0, [], [], []))
        got = r.process_rows(sa.CSRData.from_rows(rows))
        assert len(got) == len(p)
        out.append(got)
    return np.concatenate(out)


def ranked_count(ni, ban_ptr, ban_item):
    return np.array([ni - len(np.unique(ban_item[a:b])) for a, b in zip(ban_ptr[:-1], ban_ptr[1:])], np.int32)


def rule_positions(scores, pos, banned):
    """the documented rule on one section's scores"""
    on = np.ones(len(scores), bool)
    on[banned] = False
    ids = np.arange(len(scores))
    position, tied = [], []
    for p in pos:
        eq = on & (scores == scores[p]) & (ids != p)
        position.append(int((on & (scores > scores[p])).sum() + (eq & (ids < p)).sum()))
        tied.append(int(eq.sum()))
    return position, tied


@pytest.mark.parametrize("k", [1, 5, 16, 64, 100, 128, 200, 256, 320, 1024])
def test_positions_match_the_port_ranker_on_random_models(k, tmp_path):
    """517 items (a multiple of no tile), 203 sections (the last tile is ragged), every lane-group width and the wide rows; the model has been
    trained by one pass -- triples for most widths, rank pairs for k = 16 and 128 -- so its rows are not the initial draw"""
    nu, ni, S = 300, 517, 203
    if k in (16, 128):
        t = new_trainer(nu, ni, k, conf=cases.PAIR_CONF, active=3)
        t.train_dataset(t.dataset_from_pairs(*cases.planted_pairs(4000, nu, ni, seed=k)))
    else:
        t = new_trainer(nu, ni, k)
        t.train_dataset(t.dataset_from_triples(*cases.planted_triples(4000, nu, ni, seed=k)))
    lists = make_sections(S, nu, ni, seed=k)
    users, pos_ptr, pos_item, ban_ptr, ban_item = lists
    before = t.counter(38)
    position, tied, ranked, nan = t.rank_positions(*lists)
    assert t.counter(38) - before == S - 1          # every section but the one without positives
    np.testing.assert_array_equal(ranked, ranked_count(ni, ban_ptr, ban_item))
    assert ranked[30] == pos_ptr[31] - pos_ptr[30] and not nan.any()
    path = str(tmp_path / "m.model")
    t.save_model(path)
    want = port_positions(path, ni, *lists)
    assert len(want) == len(position) and (tied == 0).mean() > 0.9
    np.testing.assert_array_equal(position[tied == 0], want[tied == 0])
    # the section whose ranked candidates are its positives: the positions are a permutation of 0 .. npos - 1
    a, b = pos_ptr[30], pos_ptr[31]
    if (tied[a:b] == 0).all():
        assert sorted(position[a:b]) == list(range(b - a))


@pytest.mark.parametrize("k, ni", [pytest.param(7, 500, id="7"), pytest.param(64, 500, id="64"), pytest.param(128, 500, id="128"), pytest.param(200, 500, id="200"),
                                   pytest.param(320, 500, id="320"), pytest.param(64, 1200, id="64-1200items")])
def test_rounding_is_pinned(k, ni, tmp_path):
    """Item rows are one base row plus small perturbations (up to 800 ulp of an element, which moves a score of magnitude ~8 by a few ulp
    of the SCORE), so the scores of a section cluster within a few ulp of each other: another summation order changes positions (a plain
    sequential sum moves ~2000 of 5000 ranks on these inputs in numpy).  Condition on the input (about one half for either width when the test
    was written: 0.47 / 0.55 over every fourth user; asserted here): at least 20 % of the adjacent ranked pairs differ by less than 4 ulp in a double-precision score;
    ~3/4 of the fp32 scores are still untied, and only those positions are compared.  The widths take every sweep: k = 7, 64 and 128 two item
    tiles per pass (IB = 2), 200 one (IB = 1), 320 k_rank_eval_sweep_wide; with 1 200 items the IB = 2 sweep splits them over two workgroups in y."""
    nu, S = 40, 70
    rng = np.random.default_rng(k)
    t = new_trainer(nu, ni, k)
    base = rng.standard_normal(k).astype(F32)
    bits = np.tile(base.view(np.int32), (ni, 1)) + rng.integers(-800, 801, (ni, k)).astype(np.int32)
    W = bits.view(F32)
    U = rng.standard_normal((nu, k)).astype(F32)
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", np.zeros(ni, F32))
    lists = make_sections(S, nu, ni, seed=k + 1, big=-1, empty=-1, full_ban=-1)
    users, pos_ptr, pos_item, ban_ptr, ban_item = lists
    close = total = 0
    for s in range(0, S, 7):
        sc = np.sort(U[users[s]].astype(np.float64) @ W.astype(np.float64).T)
        ulp = np.spacing(np.abs(sc[1:]).astype(F32)).astype(np.float64)
        close += int((np.diff(sc) < 4 * ulp).sum())
        total += len(sc) - 1
    assert close >= 0.2 * total, (close, total)
    position, tied, ranked, nan = t.rank_positions(*lists)
    path = str(tmp_path / "m.model")
    t.save_model(path)
    want = port_positions(path, ni, *lists)
    assert (tied == 0).sum() >= 40 and not nan.any()
    np.testing.assert_array_equal(position[tied == 0], want[tied == 0])


@pytest.mark.parametrize("k", [7, 64])
def test_ties_follow_the_documented_rule(k):
    """small integer factors and biases: every score is exact in fp32 in any order and many are equal; positives tie with positives and with
    banned items; +0 and -0 arise on purpose (zero rows with biases of either sign of zero)"""
    nu, ni, S = 30, 200, 80
    rng = np.random.default_rng(k)
    t = new_trainer(nu, ni, k)
    W = rng.integers(-1, 2, (ni, k)).astype(F32)
    U = rng.integers(-1, 2, (nu, k)).astype(F32)
    bias = rng.integers(-1, 2, ni).astype(F32)
    W[:20] = 0.0
    W[5:10] = -0.0
    bias[:20] = np.where(np.arange(20) % 2 == 0, F32(0.0), F32(-0.0))
    W[20:30] = W[20]
    bias[20:30] = bias[20]                     # ten copies of one item
    U[3] = 0.0                                   # a user every item ties for, up to the bias
    t.set_view("W_item", W)
    t.set_view("W_user", U)
    t.set_view("i_bias", bias)
    users, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(S, nu, ni, seed=k, big=10, empty=20, full_ban=30, npos_big=150)
    users[40:44] = 3
    # sections 50 .. 59: positives and bans drawn from the zero rows and the copies, so positives tie with positives and with banned items
    pos, ban = [pos_item[a:b] for a, b in zip(pos_ptr[:-1], pos_ptr[1:])], [ban_item[a:b] for a, b in zip(ban_ptr[:-1], ban_ptr[1:])]
    for s in range(50, 60):
        pick = rng.permutation(30)
        pos[s], ban[s] = pick[:4].astype(np.uint32), pick[4:12].astype(np.uint32)
    ptr = lambda ls: np.concatenate([[0], np.cumsum([len(x) for x in ls])]).astype(np.int64)
    pos_ptr, pos_item, ban_ptr, ban_item = ptr(pos), np.concatenate(pos), ptr(ban), np.concatenate(ban)
    position, tied, ranked, nan = t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)
    assert not nan.any() and (tied > 0).mean() > 0.5
    for s in range(S):
        sc = score_fp32(U[users[s]], W, bias)
        assert np.array_equal(sc, (bias.astype(np.float64) + W.astype(np.float64) @ U[users[s]].astype(np.float64)).astype(F32))   # exact in any order
        wp, wt = rule_positions(sc, pos[s], ban[s])
        assert position[pos_ptr[s]:pos_ptr[s + 1]].tolist() == wp, s
        assert tied[pos_ptr[s]:pos_ptr[s + 1]].tolist() == wt, s


def test_nan_scores_flag_the_sections_that_rank_them():
    nu, ni, k = 20, 300, 12
    t = new_trainer(nu, ni, k)
    t.train_dataset(t.dataset_from_triples(*cases.planted_triples(2000, nu, ni, seed=1)))
    W = t.view("W_item")
    W[123] = np.nan
    t.set_view("W_item", W)
    users = np.arange(6, dtype=np.uint32)
    pos_ptr = np.array([0, 2, 4, 6, 8, 8, 10], np.int64)
    pos_item = np.array([1, 2, 3, 123, 5, 6, 7, 8, 9, 10], np.uint32)      # section 1 holds the NaN row as a positive
    ban_ptr = np.array([0, 0, 0, 2, 2, 3, 5], np.int64)
    ban_item = np.array([123, 4, 123, 123, 123], np.uint32)                 # sections 2 and 5 ban it (5 twice); 4 bans it but has no positives
    position, tied, ranked, nan = t.rank_positions(users, pos_ptr, pos_item, ban_ptr, ban_item)
    assert nan.tolist() == [1, 1, 0, 1, 0, 0]
    for s in (0, 1, 3):
        assert (position[pos_ptr[s]:pos_ptr[s + 1]] == -1).all()
    for s in (2, 5):
        assert (position[pos_ptr[s]:pos_ptr[s + 1]] >= 0).all() and ranked[s] == ni - (2 if s == 2 else 1)
    m = t.rank_eval(users, pos_ptr, pos_item, ban_ptr, ban_item, at=(5,))
    assert (m["ninst"], m["nan_sections"], m["skipped"]) == (2, 3, 1)
    assert m == sa.rank_metrics(pos_ptr, position, ranked=ranked, nan=nan, at=(5,))


def copy_model(src, dst):
    for name in ("u_bias", "W_user", "i_bias", "W_item"):
        dst.set_view(name, src.view(name))


def test_end_to_end():
    nu, ni, k, S = 120, 700, 32, 150
    u, i, r = cases.planted_triples(6000, nu, ni, seed=5)
    lists = make_sections(S, nu, ni, seed=9, big=10, empty=20, full_ban=30, npos_big=600)   # 600 positives: more than one tile of thresholds
    users, pos_ptr, pos_item, ban_ptr, ban_item = lists
    t = new_trainer(nu, ni, k)
    ds = t.dataset_from_triples(u, i, r)
    t.train_dataset(ds)
    got = t.rank_positions(*lists)                     # straight after the unsynchronised pass: it must see the trained model
    t.synchronize()
    ref = new_trainer(nu, ni, k, seed=77)
    copy_model(t, ref)                                 # the trained model, read back after a synchronise, in another handle
    want = ref.rank_positions(*lists)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    position, tied, ranked, nan = got
    assert (position >= 0).all() and (position < ranked.repeat(np.diff(pos_ptr))).all()
    # the convenience call == the metrics of its own positions == the formulas
    at = (1, 5, 10, 100)
    m = t.rank_eval(*lists, at=at)
    assert m == sa.rank_metrics(pos_ptr, position, ranked=ranked, nan=nan, at=at)
    assert m["ninst"] == S - 1 and m["skipped"] == 1
    tot, cnt = auc_restated(pos_ptr, position, ranked)
    assert (m["sum_auc"], m["nauc"]) == (tot, cnt) and cnt == S - 2        # the all-banned section has ranked == npos
    secs = [np.sort(position[a:b]) for a, b in zip(pos_ptr[:-1], pos_ptr[1:]) if b > a]
    want_map = sum(float(np.sum(np.arange(1, len(p) + 1) / (p + 1.0))) / len(p) for p in secs)
    assert abs(m["sum_map"] - want_map) <= 1e-12 * want_map                # numpy's pairwise sum against the sequential one
    assert m["sum_pre_at"][1] == sum(float((p < 5).sum()) / 5 for p in secs)
    assert m["sum_rec_at"][2] == sum(float((p < 10).sum()) / len(p) for p in secs)
    # ban_ptr = None is the same as empty ban lists
    none = t.rank_positions(users, pos_ptr, pos_item)
    empty = t.rank_positions(users, pos_ptr, pos_item, np.zeros(S + 1, np.int64), np.zeros(0, np.uint32))
    for a, b in zip(none, empty):
        np.testing.assert_array_equal(a, b)
    assert (none[2] == ni).all()
    # in pieces of whole sections: the budget lowered to 100 entries (the 600-positive section is a piece of its own)
    t.set_knob("rank_eval_budget", 100)
    for a, b in zip(t.rank_positions(*lists), got):
        np.testing.assert_array_equal(a, b)
    t.set_knob("rank_eval_budget", 1 << 22)
    # a window sequence of the same rows: the window step is not bit-equal to the exact pass, so the models are made identical through set_view
    w = new_trainer(nu, ni, k, extra=[("amd:step", "minibatch")])
    dw = w.dataset_from_triples(u, i, r)
    assert dw.kind == 8
    w.train_dataset(dw)
    gw = w.rank_positions(*lists)
    copy_model(w, ref)
    for a, b in zip(gw, ref.rank_positions(*lists)):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(gw[0], position)         # (and it IS another model)


def test_lists_are_refused_before_any_launch():
    t = new_trainer(20, 30, 8)
    with pytest.raises(sa.SvdfError, match="each pos sample item can not occur in baned sample list"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 0, 3], [1, 7, 1])
    with pytest.raises(sa.SvdfError, match="a positive item is repeated inside a section"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 5, 7])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 30, 7])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 1, 1], [4000000000])
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_positions([1, 20], [0, 2, 3], [5, 6, 7])
    assert t.counter(38) == 0
    position, tied, ranked, nan = t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 3, 5], [7, 7, 8, 5, 5])
    assert ranked.tolist() == [28, 29] and t.counter(38) == 2

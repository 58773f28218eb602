"""Live-model ranking for user-group (SVD++) trainers, the parts that need no GPU: the numpy statement of the effective user
row that tests/test_gpu_rank_feedback.py compares the GPU against, with its decoys; the conditions on the inputs that test shares (found and
asserted here, on the CPU); and every refusal of the svdf_rank_*_fb calls that is decided before the device, on a host-only handle."""
import ctypes as C

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from oracle import oracle
from rank_rounding import cluster, feature_sum, score_fp32
from test_gpu_rank_eval import make_sections, rule_positions
from test_gpu_rank_topn import make_bans
from test_rank_eval import host_trainer
from test_rank_topn import rule_topn

F32 = np.float32
ROW_DECOYS = ("fused", "reversed", "user_first")
NU, NI, NFB, NS = 120, 700, 90, 150        # two full section tiles of 64 and a ragged one
LONG, EMPTY = 40, 5                        # the section with 300 feedback entries (longer than any load batch), the one with none


def rule_user_rows(U, Wfb, users, fb_ptr, fb_index, fb_value, order="pinned"):
    """the documented rule: row s = (0 + sum_j Wfb[fid_j] * val_j, j in list order) + U[users[s]] * 1, every product and sum rounded to
    float32 (rank_rounding.feature_sum).  Decoys: "fused" product and add in float64 with one rounding, "reversed" the list backwards,
    "user_first" the user row added before the feedback."""
    fused = order == "fused"
    rows = np.zeros((len(users), U.shape[1]), F32)
    for s, u in enumerate(users):
        idx = np.asarray(fb_index[fb_ptr[s]:fb_ptr[s + 1]], np.int64)
        val = np.asarray(fb_value[fb_ptr[s]:fb_ptr[s + 1]], F32)
        if order == "reversed":
            idx, val = idx[::-1], val[::-1]
        uid, one = np.array([[int(u)]]), np.ones((1, 1), F32)
        if order == "user_first":
            f = feature_sum(Wfb, idx[None, :], val[None, :], start=feature_sum(U, uid, one))
        else:
            f = feature_sum(U, uid, one, start=feature_sum(Wfb, idx[None, :], val[None, :], fused=fused), fused=fused)
        rows[s] = f[0]
    return rows


def rule_lists(rows, W, bias, top_n, ban_ptr=None, ban_item=None):
    """Trainer.rank_topn(..., feedback=...) by the rule: section s is `user` s of the matrix of effective rows"""
    return rule_topn(rows, W, bias, np.arange(len(rows)), top_n, ban_ptr, ban_item)


def rule_pos(rows, W, bias, pos_ptr, pos_item, ban_ptr, ban_item):
    """(position, tied) of Trainer.rank_positions(..., feedback=...) by the rule (sections without NaN scores)"""
    position, tied = [], []
    for s in range(len(rows)):
        p, t = rule_positions(score_fp32(rows[s], W, bias), pos_item[pos_ptr[s]:pos_ptr[s + 1]].astype(np.int64),
                              ban_item[ban_ptr[s]:ban_ptr[s + 1]].astype(np.int64))
        position += p
        tied += t
    return np.array(position, np.int32), np.array(tied, np.int32)


def ptr_of(lists):
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)


def make_feedback(S, nfb, seed, long_at=LONG, empty_at=EMPTY, longest=40):
    """S feedback lists: 0 .. `longest` (id, value) entries each, values in (-1, 0.95) (a value within 1e-6 of 1 would multiply as 1, the
    reference's rule, which the numpy statement leaves out); every third list repeats some of its own ids; section `long_at` has 300
    entries, section `empty_at` none"""
    rng = np.random.default_rng(seed)
    idx, val = [], []
    for s in range(S):
        n = 300 if s == long_at else (0 if s == empty_at else int(rng.integers(0, longest + 1)))
        i = rng.integers(0, nfb, n)
        if s % 3 == 0 and n > 2:
            i[n // 2:] = i[:n - n // 2]           # repeated ids, added twice in order
        idx.append(i.astype(np.uint32))
        val.append(rng.uniform(-1.0, 0.95, n).astype(F32))
    return ptr_of(idx), np.concatenate(idx), np.concatenate(val)


# ---- the rounding input: clustered item rows (one base row +- 800 ulp per element, as in test_gpu_rank_topn.test_rounding_is_pinned) and
# feedback rows of mixed magnitude (1e-3 .. 10), so that the order and the fusing of the user sum move last bits of the row
_rounding = {}


def rounding_input(k):
    if k not in _rounding:
        nu, ni, nfb, S, N = 40, 500, 30, 70, 50
        rng = np.random.default_rng(100 + k)
        W = cluster(rng, ni, k, 800)
        U = rng.standard_normal((nu, k)).astype(F32)
        Wfb = (rng.standard_normal((nfb, k)) * 10.0 ** rng.uniform(-3, 1, (nfb, 1))).astype(F32)
        bias = np.zeros(ni, F32)
        users, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(S, nu, ni, seed=k + 1, big=-1, empty=-1, full_ban=-1)
        fb = make_feedback(S, nfb, seed=k + 2, long_at=-1, empty_at=-1, longest=12)
        _rounding[k] = dict(nu=nu, ni=ni, nfb=nfb, S=S, N=N, k=k, U=U, W=W, Wfb=Wfb, bias=bias, users=users, pos_ptr=pos_ptr, pos_item=pos_item,
                            ban_ptr=ban_ptr, ban_item=ban_item, fb=fb)
    return _rounding[k]


def rounding_results(c, order):
    rows = rule_user_rows(c["U"], c["Wfb"], c["users"], *c["fb"], order=order)
    return rule_lists(rows, c["W"], c["bias"], c["N"], c["ban_ptr"], c["ban_item"]), rule_pos(rows, c["W"], c["bias"], c["pos_ptr"], c["pos_item"],
                                                                                                c["ban_ptr"], c["ban_item"])


ROUNDING_KS = (64, 320)                    # a narrow width and a wide one


# ---- the port-comparison input: a model trained by one pass of user blocks through the pinned port (bit for bit what the GPU trains), the
# sections of test_gpu_rank_feedback.py
FB_CONF = dict(num_ufeedback=NFB, wd_ufeedback=0.004, ufeedback_init_sigma=0.05, ui_init_sigma=0.1)


def fb_conf(nu, ni, k, base=cases.BASICMF_CONF, **kw):
    return cases.conf_with(base, num_user=nu, num_item=ni, num_factor=k, **dict(FB_CONF, **kw))


def training_blocks(k):
    """one pass of SVD++ user blocks; at k = 16 candidate blocks with several item entries per row under the rank loss (cases.rank_blocks: its
    feedback and item ids are drawn below NFB)"""
    if k == 16:
        return cases.rank_blocks(150, NU, NFB, 0, seed=k, side_user=False)
    return cases.user_blocks(100, NU, NI, NFB, seed=k)


def section_lists(k, ni=NI):
    users, pos_ptr, pos_item, ban_ptr, ban_item = make_sections(NS, NU, ni, seed=k)
    return dict(users=users, pos_ptr=pos_ptr, pos_item=pos_item, ban_ptr=ban_ptr, ban_item=ban_item, fb=make_feedback(NS, NFB, seed=k + 7))


_port = {}


def port_input(k, top_n):
    if k not in _port:
        t = oracle.OracleTrainer("port", 1, 0)
        t.seed(3)
        for kk, v in fb_conf(NU, NI, k):
            t.set_param(kk, v)
        t.init_model()
        t.init_trainer()
        for b in training_blocks(k):
            t.update_block(b)
        c = section_lists(k)
        c.update(U=t.view("W_user").copy(), W=t.view("W_item").copy(), bias=t.view("i_bias").copy(), Wfb=t.view("W_ufeedback").copy(), N=top_n)
        t.close()
        _port[k] = c
    return _port[k]


def untied_flags(c):
    """(per section: no tie among its top_n + 1 best and at least top_n candidates; per positive: untied), from the rule alone"""
    rows = rule_user_rows(c["U"], c["Wfb"], c["users"], *c["fb"])
    more = rule_lists(rows, c["W"], c["bias"], c["N"] + 1, c["ban_ptr"], c["ban_item"])
    sec = np.array([more[2][s] >= c["N"] and (np.diff(more[1][s, :more[2][s]]) < 0).all() for s in range(len(rows))])
    _, tied = rule_pos(rows, c["W"], c["bias"], c["pos_ptr"], c["pos_item"], c["ban_ptr"], c["ban_item"])
    return sec, tied == 0


def test_the_rule_on_a_hand_made_case():
    """two users, three feedback rows, small binary fractions (every step exact): an empty list, a repeated id, a negative value"""
    U = np.array([[1, 2, 3, 4], [0.5, 0, -1, 8]], F32)
    Wfb = np.array([[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0.25, -4]], F32)
    users = [0, 1, 0]
    fb_ptr, fb_index, fb_value = [0, 0, 2, 4], [0, 0, 2, 1], np.array([0.5, 0.5, -2.0, 1.5], F32)
    want = np.array([[1, 2, 3, 4], [1.5, 0, -1, 8], [1, 5, 2.5, 12]], F32)
    for order in ("pinned",) + ROW_DECOYS:          # exact arithmetic: every order agrees
        np.testing.assert_array_equal(rule_user_rows(U, Wfb, users, fb_ptr, fb_index, fb_value, order), want)
    assert not np.signbit(rule_user_rows(np.full((1, 4), -0.0, F32), Wfb, [0], [0, 0], [], [])).any()   # 0 + (-0) * 1 = +0
    W = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], F32)
    bias = np.array([0, 0, 0, 4.5], F32)
    items, scores, count, nan = rule_lists(want, W, bias, 3, [0, 0, 1, 1], [2])
    assert items.tolist() == [[3, 2, 1], [3, 0, 1], [2, 1, 3]] and scores.tolist() == [[4.5, 4.0, 2.0], [4.5, 1.5, 0.0], [12.0, 5.0, 4.5]]
    position, tied = rule_pos(want, W, bias, np.array([0, 1, 2, 3]), np.array([1, 0, 0]), np.array([0, 0, 1, 1]), np.array([2]))
    assert position.tolist() == [2, 1, 3] and tied.tolist() == [0, 0, 0]
    fb_value[2] = np.nan                            # a NaN value reaches the whole row of its section, and only that one
    rows = rule_user_rows(U, Wfb, users, fb_ptr, fb_index, fb_value)
    assert np.isnan(rows[2, 2:]).all() and not np.isnan(rows[:2]).any()
    assert rule_lists(rows, W, bias, 3)[3].tolist() == [0, 0, 1]


@pytest.mark.parametrize("k", ROUNDING_KS)
def test_the_rounding_input_sees_every_decoy(k):
    """conditions on the input tests/test_gpu_rank_feedback.py::test_rounding_is_pinned reuses: the scores of a section lie a few ulp apart
    (at least 20 % of the adjacent sorted scores within 4 ulp), and EVERY decoy of the user sum changes the top-N list of at least one
    section and at least one position"""
    c = rounding_input(k)
    rows = rule_user_rows(c["U"], c["Wfb"], c["users"], *c["fb"])
    close = total = 0
    for s in range(0, c["S"], 7):
        sc = np.sort(rows[s].astype(np.float64) @ c["W"].astype(np.float64).T)
        ulp = np.spacing(np.abs(sc[1:]).astype(F32)).astype(np.float64)
        close += int((np.diff(sc) < 4 * ulp).sum())
        total += len(sc) - 1
    assert close >= 0.2 * total, (close, total)
    (items, _, count, nan), (position, tied) = rounding_results(c, "pinned")
    assert not nan.any() and (count == c["N"]).all()
    for decoy in ROW_DECOYS:
        (ditems, _, _, _), (dposition, _) = rounding_results(c, decoy)
        assert (ditems != items).any(axis=1).sum() >= 1, decoy
        assert (dposition != position).sum() >= 1, decoy


@pytest.mark.parametrize("k, top_n", [(64, 10), (128, 100)])
def test_the_port_comparison_input_is_mostly_untied(k, top_n):
    """what the comparison with the port's ranker relies on: at least 90 % of the sections have no tie among their top_n + 1 best, at least
    90 % of the positives are untied -- and the feedback rows are not their initial draw"""
    c = port_input(k, top_n)
    sec, pos = untied_flags(c)
    assert sec.mean() >= 0.9 and pos.mean() >= 0.9, (sec.mean(), pos.mean())
    fresh = oracle.OracleTrainer("port", 1, 0)
    fresh.seed(3)
    for kk, v in fb_conf(NU, NI, k):
        fresh.set_param(kk, v)
    fresh.init_model()
    assert not np.array_equal(fresh.view("W_ufeedback"), c["Wfb"])
    fresh.close()


def test_the_feedback_lists_cover_what_the_issue_names():
    fb_ptr, fb_index, fb_value = make_feedback(NS, NFB, seed=71)
    n = np.diff(fb_ptr)
    assert n[LONG] == 300 and n[EMPTY] == 0 and set(range(0, 41)) >= set(np.delete(n, LONG).tolist()) and n.max() == 300
    assert any(len(np.unique(fb_index[a:b])) < b - a for a, b in zip(fb_ptr[:-1], fb_ptr[1:]))
    assert (fb_value < 0).any() and (np.abs(fb_value - 1) > 1e-3).all()


# ---- refusals on host-only handles
def group_trainer(ext=0, extra=(), **kw):
    return host_trainer(fmt=1, ext=ext, extra=[("num_ufeedback", 30)] + list(extra), **kw)


USERS, POS = [1, 2], ([0, 2, 3], [5, 6, 7])
FB = ([0, 2, 3], [3, 29, 4], [0.5, -1.0, 2.0])


def calls(t, fb):
    """the three methods with one feedback argument"""
    return [lambda: t.rank_positions(USERS, *POS, feedback=fb), lambda: t.rank_eval(USERS, *POS, feedback=fb), lambda: t.rank_topn(USERS, 5, feedback=fb)]


@pytest.mark.parametrize("ext", [0, 1])
def test_a_legal_call_on_a_host_only_user_group_handle_needs_a_gpu(ext):
    t = group_trainer(ext)
    for call in calls(t, FB):
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call()
    legal = ([0, 0, 4], [7, 7, 0, 7], [np.nan, -0.0, 1e30, 0.5])      # an empty list, a repeated id, any float value
    for call in calls(t, legal):
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call()
    with pytest.raises(sa.SvdfError, match="rank_topn needs a GPU"):
        t.rank_topn([1, 1], 5, feedback=([0, 1, 3], [3, 4, 5], [1.0, 1.0, 1.0]))   # a user in two sections with different lists
    assert t.counter(40) == 0


def test_feedback_list_refusals_come_before_the_device():
    t = group_trainer()
    for j, who in enumerate(("rank_eval", "rank_eval", "rank_topn")):       # rank_positions, rank_eval, rank_topn
        call = lambda fb, j=j: calls(t, fb)[j]()
        with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
            call(([0, 2, 3], [3, 30, 4], [0.5, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match="ufeedback id exceed bound"):
            call(([0, 2, 3], [3, 4000000000, 4], [0.5, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": fb_ptr must not decrease"):
            call(([0, 3, 2], [3, 29, 4], [0.5, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": fb_ptr must start at >= 0"):
            call(([-1, 2, 3], [3, 29, 4], [0.5, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": fb_ptr must have one entry more than users"):
            call(([0, 3], [3, 29, 4], [0.5, -1.0, 2.0]))
        with pytest.raises(sa.SvdfError, match=who + ": fb_ptr is NULL on a user-group trainer.*explicitly as an empty list"):
            call((None, None, None))
    # fb_ptr with entries but without fb_index / fb_value: through the C entry points
    users, ptr = np.array(USERS, np.uint32), np.array(FB[0], np.int64)
    idx, val = np.array(FB[1], np.uint32), np.array(FB[2], F32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    items, count, nan = np.zeros(10, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    for fb_index, fb_value in ((None, p(val)), (p(idx), None)):
        assert t.lib.svdf_rank_topn_fb(t.h, 2, users, p(ptr), fb_index, fb_value, None, None, 5, items, None, count, nan) == -1
        assert "rank_topn: fb_index / fb_value is missing" in t.lib.svdf_last_error().decode()
        pos_ptr, pos_item, out = np.array(POS[0], np.int64), np.array(POS[1], np.uint32), [np.zeros(3, np.int32) for _ in range(4)]
        assert t.lib.svdf_rank_eval_positions_fb(t.h, 2, users, p(ptr), fb_index, fb_value, pos_ptr, pos_item, None, None, *out) == -1
        assert "rank_eval: fb_index / fb_value is missing" in t.lib.svdf_last_error().decode()
    # the other lists are still refused in their own words
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_topn([1, 20], 5, feedback=FB)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions(USERS, [0, 2, 3], [5, 30, 7], feedback=FB)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
        t.rank_topn(USERS, 257, feedback=FB)
    assert t.counter(38) == t.counter(39) == t.counter(40) == 0


def test_configuration_refusals_of_the_feedback_calls(tmp_path):
    # lists on a format_type = 0 trainer; without lists the _fb call IS the old call
    t0 = host_trainer()
    for call in calls(t0, FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): feedback lists need a user-group trainer"):
            call()
    for call in calls(t0, (None, None, None)):
        with pytest.raises(sa.SvdfError, match="needs a GPU"):
            call()
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t0.rank_topn([1, 20], 5, feedback=(None, None, None))
    # feedback=None on a user-group handle calls the old functions: today's message
    for ext in (0, 1):
        for call in calls(group_trainer(ext), None):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): user-group trainers .*are not covered: the score has a feedback part"):
                call()
    # what neither route covers, in today's words
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    for key in ("feature_user", "feature_item"):
        for call in calls(group_trainer(extra=[(key, str(table))]), FB):
            with pytest.raises(sa.SvdfError, match="rank_(eval|topn): .*side tables change the score"):
                call()
    for call in calls(group_trainer(extra=[("amd:gpus", 2)]), FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): amd:gpus > 1 is not covered"):
            call()
    for call in calls(host_trainer(fmt=1, nu=30, extra=[("num_ufeedback", 30), ("common_latent_space", 1), ("common_feedback_space", 1)]), FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): common_latent_space != 0"):
            call()


@pytest.mark.parametrize("ext", [2, 15])
def test_other_extend_types_are_refused_in_todays_words(ext):
    t = sa.Trainer(1, 0, ext, device=-2)
    for call in calls(t, FB):
        with pytest.raises(sa.SvdfError, match="rank_(eval|topn): user-group trainers .*extend_type != 0 are not covered"):
            call()

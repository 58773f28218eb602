"""Batch ranking evaluation, the parts that need no GPU: svdf_rank_eval_metrics against tests/golden/rank_eval.npz -- the sums
of the reference's own EvaluatorMAP (apex-utils/apex_evaluator.h), recorded by tests/golden/make_rank_eval_golden.py -- the AUC against a
restatement, and every refusal of svdf_rank_eval_positions that is decided before the device, on a host-only handle."""
import os

import numpy as np
import pytest

import cases
import svdfeature_amd as sa

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank_eval.npz")


def gold_case(name):
    g = np.load(GOLD)
    return {k: g[name + "_" + k] for k in ("at", "sec_ptr", "position", "ranked", "text", "ninst", "sums")}


def print_result_text(m):
    """EvaluatorMAP::print_result (apex_evaluator.h:194-207) over the sums the library returns"""
    n = m["ninst"]
    s = "MAP:%f" % (m["sum_map"] / n)
    for name, key in (("MAP", "sum_map_at"), ("Pre", "sum_pre_at"), ("Rec", "sum_rec_at")):
        for k, v in zip(m["at"], m[key]):
            s += " %s@%d:%f" % (name, k, v / n)
    return s


@pytest.mark.parametrize("name", ["all", "long", "pairs"])
def test_metrics_equal_the_reference_evaluator(name):
    """the raw sums to the last bit (the fixture holds them as hex floats of the reference's doubles) and the %f line print_result writes;
    `all` lists its cut-offs unsorted -- they are handled in ascending order like init() does -- and its lists are not sorted either"""
    g = gold_case(name)
    m = sa.rank_metrics(g["sec_ptr"], g["position"], at=tuple(int(k) for k in g["at"]))
    assert m["at"] == sorted(int(k) for k in g["at"])
    assert m["ninst"] == int(g["ninst"]) and m["skipped"] == 0
    got = np.array([m["sum_map"]] + m["sum_map_at"] + m["sum_pre_at"] + m["sum_rec_at"], np.float64)
    np.testing.assert_array_equal(got.view(np.uint64), g["sums"].view(np.uint64))
    assert print_result_text(m) == str(g["text"])


def test_fixture_covers_what_the_issue_names():
    g = gold_case("all")
    n = np.diff(g["sec_ptr"])
    assert 290 <= len(n) <= 320 and {1, 2, 17, 300} <= set(n.tolist())
    assert sorted(g["at"].tolist()) == [1, 5, 10, 100]
    assert (g["position"] == 0).any() and (g["position"] == g["ranked"][0] - 1).any()


def test_unsorted_positions_are_sorted_by_the_function():
    g = gold_case("all")
    ptr, pos = g["sec_ptr"], g["position"].copy()
    assert any((np.diff(pos[a:b]) < 0).any() for a, b in zip(ptr[:-1], ptr[1:]))   # the fixture's lists are not sorted ...
    srt = pos.copy()
    for a, b in zip(ptr[:-1], ptr[1:]):
        srt[a:b] = np.sort(pos[a:b])
    rev = pos.copy()
    for a, b in zip(ptr[:-1], ptr[1:]):
        rev[a:b] = np.sort(pos[a:b])[::-1]
    ms = [sa.rank_metrics(ptr, p, at=(1, 5, 10, 100)) for p in (pos, srt, rev)]
    assert ms[0] == ms[1] == ms[2]                                                   # ... and any order inside a section gives the same bits
    assert np.array_equal(pos, g["position"])                                        # the caller's array is left alone


def auc_restated(ptr, pos, ranked):
    tot, cnt = 0.0, 0
    for s, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        n = int(b - a)
        if n == 0 or int(ranked[s]) == n:
            continue
        p = np.sort(pos[a:b]).astype(np.int64)
        above = int((p - np.arange(n)).sum())
        tot += 1.0 - float(above) / (float(n) * float(int(ranked[s]) - n))
        cnt += 1
    return tot, cnt


@pytest.mark.parametrize("name", ["all", "long", "pairs"])
def test_auc_equals_a_numpy_restatement(name):
    g = gold_case(name)
    m = sa.rank_metrics(g["sec_ptr"], g["position"], ranked=g["ranked"])
    tot, cnt = auc_restated(g["sec_ptr"], g["position"], g["ranked"])
    assert m["nauc"] == cnt and m["sum_auc"] == tot
    if name == "all":
        assert cnt == m["ninst"] - 1          # the list with ranked == npos is skipped by the AUC alone
    assert "AUC" in m and 0.0 <= m["AUC"] <= 1.0
    assert "AUC" not in sa.rank_metrics(g["sec_ptr"], g["position"])   # no `ranked`, no AUC


def test_auc_extremes_and_sections_that_are_no_instances():
    # positives on top: AUC 1; at the bottom: 0; an empty section and a flagged one are no instances
    ptr = np.array([0, 2, 4, 4, 6], np.int64)
    pos = np.array([1, 0, 9, 8, -1, -1], np.int32)
    m = sa.rank_metrics(ptr, pos, ranked=[10, 10, 10, 10], nan=[0, 0, 0, 1], at=(1,))
    assert (m["ninst"], m["skipped"], m["nan_sections"], m["nauc"]) == (2, 1, 1, 2)
    assert m["sum_auc"] == 1.0 + 0.0
    assert m["sum_pre_at"] == [1.0] and m["sum_rec_at"] == [0.5]
    with pytest.raises(sa.SvdfError, match="negative position"):
        sa.rank_metrics(ptr, pos, at=(1,))
    with pytest.raises(sa.SvdfError, match="up to 8 cut-offs"):
        sa.rank_metrics(ptr, pos, nan=[0, 0, 0, 1], at=tuple(range(1, 10)))


def host_trainer(fmt=0, ext=0, extra=(), nu=20, ni=30):
    t = sa.Trainer(fmt, 0, ext, device=-2)
    for k, v in cases.conf_with(cases.BASICMF_CONF, num_user=nu, num_item=ni, num_factor=8) + list(extra):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


LISTS = ([1, 2], [0, 2, 3], [5, 6, 7])   # users, pos_ptr, pos_item


def test_refusals_that_need_no_device(tmp_path):
    with pytest.raises(sa.SvdfError, match="needs a GPU"):
        host_trainer().rank_positions(*LISTS)
    with pytest.raises(sa.SvdfError, match="user-group trainers"):
        host_trainer(fmt=1, extra=[("num_ufeedback", 30)]).rank_positions(*LISTS)
    with pytest.raises(sa.SvdfError, match="extend_type != 0"):
        host_trainer(fmt=1, ext=1, extra=[("num_ufeedback", 30)]).rank_eval(*LISTS)
    with pytest.raises(sa.SvdfError, match="common_latent_space != 0"):
        host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]).rank_positions(*LISTS)
    with pytest.raises(sa.SvdfError, match="amd:gpus > 1 is not covered"):
        host_trainer(extra=[("amd:gpus", 2)]).rank_positions(*LISTS)
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    for key in ("feature_user", "feature_item"):
        with pytest.raises(sa.SvdfError, match="side tables change the score"):
            host_trainer(extra=[(key, str(table))]).rank_positions(*LISTS)


def test_list_refusals_come_before_the_device():
    """the ranker's messages, raised while validating on the host: a host-only handle gets them, not `needs a GPU`"""
    t = host_trainer()
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_positions([1, 20], [0, 2, 3], [5, 6, 7])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 30, 7])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 1, 1], [30])
    with pytest.raises(sa.SvdfError, match="each pos sample item can not occur in baned sample list"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 0, 3], [1, 7, 1])
    with pytest.raises(sa.SvdfError, match="a positive item is repeated inside a section"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 5, 7])
    with pytest.raises(sa.SvdfError, match="pos_ptr must not decrease"):
        t.rank_positions([1, 2], [0, 2, 1], [5, 6, 7])
    with pytest.raises(sa.SvdfError, match="one entry more than users"):
        t.rank_positions([1, 2], [0, 2], [5, 6])
    # the same item as a positive of one section and banned in another, and a ban list with duplicates, are legal: only the device is missing
    with pytest.raises(sa.SvdfError, match="needs a GPU"):
        t.rank_positions([1, 2], [0, 2, 3], [5, 6, 7], [0, 3, 5], [7, 7, 8, 5, 5])

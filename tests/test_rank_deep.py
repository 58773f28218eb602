"""Deep top-N lists (knob rank_topn_deep, top_n 257 .. 4096) without a GPU: the knob, what it admits, the probe's deep geometry."""
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from test_rank_eval import host_trainer
from test_rank_geometry import probe_handle


def deep_geometry(k, num_item, nsec, top_n, budget, matrix):
    """tests/rank_geometry.py's rule (matrix: at the width of rows of up to 128 floats) with lists of 2 top_n keys in whole 128s at every width"""
    cap = -(-2 * top_n // 128) * 128
    g = rg.topn_geometry(min(k, 128) if matrix else k, num_item, nsec, 256, budget // cap * 512)   # top_n 256: as many lists of 512 keys
    return dict(g, cap=cap)


@pytest.mark.parametrize("call, who", [(lambda t, n: t.rank_topn([1, 2], n), "rank_topn"), (lambda t, n: t.similar_items([1, 2], n), "item_topn")])
def test_what_the_knob_admits(call, who):
    t = host_trainer()
    with pytest.raises(sa.SvdfError, match=who + ": top_n must be between 1 and 256"):
        call(t, 257)
    for v in (-1, 2):
        with pytest.raises(sa.SvdfError, match=r"rank_topn_deep must be 0 or 1"):
            t.set_knob("rank_topn_deep", v)
    for v in (1, 0, 1):
        t.set_knob("rank_topn_deep", v)
    for n in (256, 257, 4096):                         # admitted: only the device is missing
        with pytest.raises(sa.SvdfError, match=who + " needs a GPU"):
            call(t, n)
    for n in (4097, 1 << 20, 0):
        with pytest.raises(sa.SvdfError, match=who + ": top_n must be between 1 and 4096.*svdf_ranker_.*top_k"):
            call(t, n)
    assert t.counter(61) == 0


@pytest.mark.parametrize("k, matrix", [(64, 0), (320, 0), (64, 1), (320, 1)])
def test_the_probe_answers_the_deep_capacity(k, matrix):
    """a narrow and a wide width, pinned and matrix: top_n at both ends, either side of a whole 128 of 2 top_n, 4032 (8064 keys) and 4096"""
    t = probe_handle(k, 1)
    t.set_knob("rank_topn_scores", matrix)
    t.set_knob("rank_topn_prefilter", 1)               # no effect on a deep call
    shallow = {}
    for ni in (129, 5000, 100000):
        t.set_param("num_item", str(ni))
        for units in (1, 65, 10000):
            for budget in (rg.TOPN_BUDGET, 1 << 16):
                t.set_knob("rank_topn_budget", budget)
                t.set_knob("rank_topn_deep", 0)
                with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256"):
                    t.rank_geometry("topn", units, 257)
                for n in (1, 100, 256):
                    shallow[ni, units, budget, n] = t.rank_geometry("topn", units, n)
                t.set_knob("rank_topn_deep", 1)
                for n in (1, 100, 256):                # top_n <= 256: the knob changes nothing
                    assert t.rank_geometry("topn", units, n) == shallow[ni, units, budget, n]
                for n in (257, 320, 321, 1000, 4032, 4033, 4096):
                    got, want = t.rank_geometry("topn", units, n), deep_geometry(k, ni, units, n, budget, matrix)
                    assert got == want and n + 128 <= got["cap"] <= 8192, (ni, units, budget, n, got, want)
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 4096"):
        t.rank_geometry("topn", 1, 4097)

"""The knobs rank_topn_prefilter and rank_topn_prefilter_slack, the parts that need no GPU: their values, and the launch
geometry the probe svdf_rank_geometry answers under them -- the matrix sweep's rule at top_n + slack."""
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from test_rank_geometry import probe_handle


def test_the_knobs_and_their_refusals():
    t = probe_handle(64, 1000)
    for v in (0, 1, 0):
        t.set_knob("rank_topn_prefilter", v)
    for v in (-1, 2):
        with pytest.raises(sa.SvdfError, match=r"rank_topn_prefilter must be 0 or 1"):
            t.set_knob("rank_topn_prefilter", v)
    for v in (1, 128, 32):
        t.set_knob("rank_topn_prefilter_slack", v)
    for v in (0, 129, -5):
        with pytest.raises(sa.SvdfError, match=r"rank_topn_prefilter_slack must be between 1 and 128"):
            t.set_knob("rank_topn_prefilter_slack", v)
    assert (t.counter(51), t.counter(52)) == (0, 0)


@pytest.mark.parametrize("k, ni, units, n, slack", [(8, 517, 70, 10, 32), (128, 100000, 10000, 100, 32), (320, 3585, 1000, 256, 128),
                                                    (1024, 20000, 5000, 1, 1), (64, 129, 200000, 193, 7)])
def test_the_probe_follows_the_knobs(k, ni, units, n, slack):
    t = probe_handle(k, ni)
    t.set_knob("rank_topn_prefilter_slack", slack)
    for budget in (rg.TOPN_BUDGET, 1 << 14):
        t.set_knob("rank_topn_budget", budget)
        assert t.rank_geometry("topn", units, n) == rg.topn_geometry(k, ni, units, n, budget)       # the prefilter at 0: unchanged
        t.set_knob("rank_topn_prefilter", 1)
        assert t.rank_geometry("topn", units, n) == rg.topn_geometry(min(k, 128), ni, units, n + slack, budget)
        t.set_knob("rank_topn_scores", 1)                                                           # the matrix mode takes precedence
        assert t.rank_geometry("topn", units, n) == rg.topn_geometry(min(k, 128), ni, units, n, budget)
        t.set_knob("rank_topn_scores", 0)
        t.set_knob("rank_topn_prefilter", 0)

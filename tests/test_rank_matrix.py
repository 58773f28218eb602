"""The knob rank_topn_scores, the parts that need no GPU: its values, and the launch geometry the probe svdf_rank_geometry
answers under it -- with 0 the rule of tests/rank_geometry.py, with 1 the matrix sweep's, stated below."""
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from test_rank_geometry import probe_handle


def matrix_geometry(k, *rest):
    """the matrix sweep: at EVERY width what the pinned rule says of rows of up to 128 floats -- tiles of 128 items, 64 sections per workgroup,
    about 2048 workgroups, room for top_n kept keys plus 128 appends; pieces as before"""
    return rg.topn_geometry(min(k, 128), *rest)


def test_the_knob_takes_0_and_1():
    t = probe_handle(64, 1000)
    for v in (0, 1, 0):
        t.set_knob("rank_topn_scores", v)
    for v in (-1, 2):
        with pytest.raises(sa.SvdfError, match=r"rank_topn_scores must be 0 \(pinned\) or 1 \(matrix\)"):
            t.set_knob("rank_topn_scores", v)


@pytest.mark.parametrize("k", [8, 128, 132, 256, 260, 1024])
def test_the_probe_follows_the_knob(k):
    t = probe_handle(k, 1)
    for ni in (1, 127, 128, 129, 517, 3585, 20000, 100000):
        t.set_param("num_item", str(ni))
        for units in (1, 64, 65, 5000, 200000):
            for budget in (rg.TOPN_BUDGET, 1 << 14):
                t.set_knob("rank_topn_budget", budget)
                for n in (1, 64, 65, 192, 193, 256):
                    t.set_knob("rank_topn_scores", 1)
                    assert t.rank_geometry("topn", units, n) == matrix_geometry(k, ni, units, n, budget), (ni, units, n, budget)
                    t.set_knob("rank_topn_scores", 0)
                    assert t.rank_geometry("topn", units, n) == rg.topn_geometry(k, ni, units, n, budget), (ni, units, n, budget)

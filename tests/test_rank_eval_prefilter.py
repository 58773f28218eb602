"""The knobs rank_eval_prefilter and rank_eval_prefilter_band, the parts that need no GPU: their values, and the launch
geometry the probe svdf_rank_geometry answers for the mode the handle is in -- rows of 28 sorted positives in units of 64 under the
matrix sweep's rule, a row's band list counted into the piece budget."""
import numpy as np
import pytest

import rank_geometry as rg
import svdfeature_amd as sa
from test_rank_geometry import probe_handle

ROW_POS = 28


def test_the_knobs_and_their_refusals():
    t = probe_handle(64, 1000)
    for v in (0, 1, 0):
        t.set_knob("rank_eval_prefilter", v)
    for v in (-1, 2):
        with pytest.raises(sa.SvdfError, match=r"rank_eval_prefilter must be 0 or 1"):
            t.set_knob("rank_eval_prefilter", v)
    for v in (64, 65536, 1024):
        t.set_knob("rank_eval_prefilter_band", v)
    for v in (63, 65537, -1):
        with pytest.raises(sa.SvdfError, match=r"rank_eval_prefilter_band must be between 64 and 65536"):
            t.set_knob("rank_eval_prefilter_band", v)
    assert (t.counter(53), t.counter(54)) == (0, 0)


@pytest.mark.parametrize("k, ni, S, band, budget", [(8, 2177, 70, 1024, rg.EVAL_BUDGET), (128, 100000, 10000, 1024, rg.EVAL_BUDGET),
                                                    (320, 3585, 1000, 64, 1 << 14), (1024, 517, 200, 65536, 1 << 20)])
def test_the_probe_answers_for_the_mode(k, ni, S, band, budget):
    npos = np.random.default_rng(k).integers(0, 6, S)
    npos[S // 2] = 300
    pos_ptr = np.concatenate([[0], np.cumsum(npos)]).astype(np.int64)
    t = probe_handle(k, ni)
    t.set_knob("rank_eval_budget", budget)
    t.set_knob("rank_eval_prefilter_band", band)
    assert t.rank_geometry("positions", S, pos_ptr=pos_ptr) == rg.eval_geometry(k, ni, pos_ptr=pos_ptr, budget=budget)   # the knob at 0: unchanged
    t.set_knob("rank_eval_prefilter", 1)
    rows = -(-npos // ROW_POS)
    load = np.cumsum(npos + 1 + rows * (band + 2))
    piece = max(1, int(np.searchsorted(load, budget, side="right")))
    nrow = int(rows[:piece].sum())
    gy, per = rg._split(ni, 128, -(-nrow // 64), 2048)
    assert t.rank_geometry("positions", S, pos_ptr=pos_ptr) == dict(gy=gy, items_per_block=per, cap=band, tile_rows=64, rows=nrow, tiles=-(-nrow // 64),
                                                                    sections=piece, launches=1)

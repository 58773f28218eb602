"""The checker of the window step with shared user rows (tests/shared_user_sim.py) pinned to the existing window checker: on rows with one
user entry (and global entries) it must equal oracle update_batch_stale followed by the window's add (multi_rank_utils.OracleShard), bit for
bit, over several windows and passes.  CPU only."""
import numpy as np
import pytest

import cases
import shared_user_sim
from multi_rank_utils import OracleShard

NU, NI, NG = 40, 30, 12


@pytest.mark.parametrize("k,active,reg,extra", [(8, 0, 0, ()), (16, 2, 1, (("no_user_bias", "1"),)), (7, 0, 3, (("user_nonnegative", "1"),)),
                                                (5, 0, 2, (("up:wd", "0.01"), ("up:bound", "20"), ("up:wd", "0.002"), ("up:bound", str(NU))))])
def test_checker_equals_the_stale_step_on_rows_with_one_user_entry(k, active, reg, extra):
    conf = cases.conf_with(cases.BASICMF_CONF, num_user=NU, num_item=NI, num_global=NG, num_factor=k, reg_method=reg,
                           wd_global="0.002", learning_rate="0.01") + list(extra)
    if active == 2:
        conf = cases.conf_with(conf, base_score="0.5")
    rng = np.random.default_rng(k)
    d = shared_user_sim.shared_rows(rng, 240, NU, 0, NI, num_global=NG, max_g=3, max_shared=0, uvals=True)
    if active == 2:
        d.row_label[:] = (rng.random(d.num_row) < 0.5).astype(np.float32)
    ub = dict(extra).get("no_user_bias", "0") != "1"
    a = shared_user_sim.make_oracle(conf, active=active)
    b = OracleShard(shared_user_sim.make_oracle(conf, active=active), minibatch=True)
    W = 4
    for _ in range(2):
        for b0, b1 in shared_user_sim.window_cuts(d.num_row, W):
            win = d.slice_rows(b0, b1)
            shared_user_sim.window_step(a, win, NU, ub)
            b.train(win)
            b.delta_set(b.delta_get())
    for name in ("W_user", "u_bias", "W_item", "i_bias", "g_bias"):
        x, y = a.view(name), b.t.view(name)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name

"""The inputs of tests/test_gpu_fuzz_wunit.py, checked without a GPU: the same seeds and counts through fuzz_wunit.draw and the oracle-backed
simulation.  (a) every simulated parameter of every draw is finite -- the script compares NaN with NaN as equal, which would hide a difference in a
diverged run; (b) the twelve wide draws reach what the slice is there for.  Conditions on the inputs, not on the engine."""
import numpy as np
import pytest

import fuzz_wunit
from test_gpu_fuzz_wunit import SLICES


@pytest.fixture(scope="module")
def drawn():
    from oracle import oracle
    oracle.build()
    out = {}
    for mode, (kw, seed, draws) in SLICES.items():
        rng = np.random.default_rng(seed)
        out[mode] = []
        for _ in range(draws):
            d = fuzz_wunit.draw(rng, **kw)
            sim = fuzz_wunit.simulate_draw(d)
            finite = all(bool(np.isfinite(s.t.view(name)).all()) for s in sim for name in d["names"])
            out[mode].append((d["desc"], d["plan"], finite))
            del d, sim
    return out


def test_the_slices_are_the_sizes_the_suite_names():
    assert {mode: n for mode, (_, _, n) in SLICES.items()} == {"wide": 12, "one_gpu": 10, "wave": 10, "ranks": 10}


@pytest.mark.parametrize("mode", list(SLICES))
def test_every_simulated_model_of_a_slice_is_finite(drawn, mode):
    assert len(drawn[mode]) == SLICES[mode][2]
    for case, (desc, _, finite) in enumerate(drawn[mode]):
        assert finite, (case, desc)


def test_the_wide_slice_covers_every_row_width_class_and_both_knob_settings(drawn):
    descs = [x[0] for x in drawn["wide"]]
    plans = [x[1] for x in drawn["wide"]]
    ks = [d["k"] for d in descs]
    assert all(k in fuzz_wunit.WIDE_WIDTHS and 256 < k <= 1024 for k in ks)
    assert all(p["onegpu"] and p["world"] == 1 for p in plans)
    per_lane = [(k + 255) // 256 for k in ks]   # float4 per lane of WideRow<V> (svdf_device.h)
    for v in (2, 3, 4):
        assert per_lane.count(v) >= 2, (v, ks)
    assert sum(k % 4 != 0 for k in ks) >= 3, ks
    assert sum(bool(d["blocks"]) for d in descs) >= 3 and sum(not d["blocks"] for d in descs) >= 3
    assert sum(bool(d["bf16"]) for d in descs) >= 2
    assert sum(d["active"] != 0 for d in descs) >= 2 and {d["active"] for d in descs} <= {0, 1, 2, 5}
    assert any(p["inplace"] == 0 for p in plans) and any(p["defer"] == 0 for p in plans)

"""Short slices of tests/fuzz_wunit.py, the randomised differential run of the user-unit window kernels (svdf_k_wunit.hip) against
tests/multi_rank_utils.simulate: every mode of the script with a fixed seed, every draw exact on uint32 views.  The wide slice (--wide: widths
257 .. 1024, links 0 / 1 / 2 / 5) also scores each trained data set against predict_batch / predict_block of the same trainer.
tests/test_fuzz_wunit_draws.py runs the same draws on the CPU: every simulated model is finite (the script treats NaN == NaN as a match), and the
wide slice reaches every WideRow<V>, ragged widths, both shapes, bf16 slots, non-linear links and both settings of the two knobs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# mode -> (keyword arguments of fuzz_wunit.draw, seed, draws)
SLICES = {
    "wide": (dict(wide=True), 1, 12),
    "one_gpu": (dict(onegpu=True), 1, 10),
    "wave": (dict(wave=True), 1, 10),
    "ranks": (dict(), 1, 10),
}


@pytest.fixture(scope="module", autouse=True)
def _port():
    from oracle import oracle
    oracle.build()


@pytest.mark.parametrize("mode", list(SLICES))
def test_a_slice_of_the_user_unit_fuzz_is_exact(mode):
    import torch
    import fuzz_wunit
    kw, seed, draws = SLICES[mode]
    rng = np.random.default_rng(seed)
    failed = []
    for case in range(draws):
        d = fuzz_wunit.draw(rng, **kw)
        if not fuzz_wunit.run(d, torch):
            failed.append((case, d["desc"]))
    assert not failed, failed

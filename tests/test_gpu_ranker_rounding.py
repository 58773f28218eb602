"""The ranker (svdf_ranker_*, svdf_k_rank.hip) on inputs whose rank order depends on the last bit of a score (tests/rank_rounding.py): every
integer it returns against the CPU checker, index for index.  The scores of a section lie a few ulp apart, so a kernel that sums in another
order, contracts a multiply-add or fuses an axpy of the candidate preparation or the user sum fails here; tests/test_rank_rounding.py proves
on the CPU that every such decoy changes at least five compared outputs of every case.  The tests on random or trained models
(test_gpu_ranker.py, fuzz_ranker.py, the goldens) cannot see any of that: their scores lie thousands of ulp apart.

With the compiled reference at hand ALL outputs are compared, ties included (tied sections are finished on the host from the device's scores, in
the reference's sort order); otherwise the untied outputs against the pinned port.

What runs, by case (rank_rounding.CASES) and route -- "tiles" = one process_rows call per group of sections, "single" = the same with
amd:rank_tile = 0, "lines" = one process call per line.  The first section after the candidates arrive is always scored alone.
  pos_k*    positions at every width; tiles: k_rank_tile_open + k_rank_score_tile<8, 0> (a full tile of 32, 4 per wave) and <4, 0>;
            single: k_rank_user + k_rank_score<8, 1>
  top10_k*  tiles of 2 / 7 / 13 sections: k_rank_score_tile<4 | 8 | 16, 1> + k_rank_tile_select; single: k_rank_score<8, 2> + radix selection
  top40_k*  the radix selection of a whole tile
  many_k*   a section with 70 positives (more than one wave of them)
  bans_k*, top10_bans_k64   25 banned candidates in every section
  spec_k*   special samples for half of the candidates: k_rank_spec + k_rank_score<8, 0> on item_score + k_rank_positions
  prep_k*   two-feature candidates and users: rank_prepare_item, the transpose, the user sum
  sort_k64  top 2 100 of 2 400: the device sort
  group_k16 a user-group model, sections in blocks with a feedback list: k_rank_feedback
  and, in a child process with SVDF_RANK_SECS_PER_WAVE = 32, k_rank_score_tile<32, 0 | 1>"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rank_rounding as rr
import svdfeature_amd as sa
from oracle import oracle

pytestmark = pytest.mark.gpu

ROUTES = {"tiles": ("rows", ()), "single": ("rows", (("amd:rank_tile", "0"),)), "lines": ("lines", ())}


def checker(c, path):
    """(wanted outputs, the flags of those that are compared)"""
    if oracle.have_reference():
        want, _ = c.run(lambda f: oracle.OracleRanker("reference", f, 0), path)
        return c.per_output(want), np.ones(len(c.per_output(want)), bool)
    want, _ = c.run(lambda f: oracle.OracleRanker("port", f, 0), path)
    return c.per_output(want), c.compared(c.scores())


def check(name, tmp_path, routes):
    c = rr.case(name)
    path = c.write_model(str(tmp_path / "m.model"))
    want, sel = checker(c, path)
    for route in routes:
        how, params = ROUTES[route]
        got, r = c.run(lambda f: sa.Ranker(f, 0), path, how=how, params=params)
        assert r.counter(0) == c.nsec
        if route == "tiles":
            assert r.counter(3) >= len(c.groups)          # every group of sections made at least one tile
        else:
            assert r.counter(3) == 0
        got = c.per_output(got)
        assert got.shape == want.shape, route
        bad = np.flatnonzero((got != want).any(1) & sel)
        assert bad.size == 0, "%s / %s: %d of %d compared outputs differ, first %s: %s != %s" % (
            name, route, bad.size, int(sel.sum()), bad[:5], got[bad[:5]].tolist(), want[bad[:5]].tolist())
        r.close()


@pytest.mark.parametrize("k", rr.WIDTHS)
def test_positions(k, tmp_path):
    check("pos_k%d" % k, tmp_path, ("tiles", "single") + (("lines",) if k == 64 else ()))


@pytest.mark.parametrize("k", rr.SOME)
@pytest.mark.parametrize("what", ["top10", "top40", "many", "bans"])
def test_prefixes_long_lists_and_bans(what, k, tmp_path):
    check("%s_k%d" % (what, k), tmp_path, ("tiles", "single"))


@pytest.mark.parametrize("name", ["top10_bans_k64", "top10_long_k64"])
def test_prefixes_with_bans_and_full_tiles(name, tmp_path):
    check(name, tmp_path, ("tiles", "single"))


@pytest.mark.parametrize("k", rr.SOME)
def test_special_samples(k, tmp_path):
    """sections with special samples are never tiled: one process_rows call scores them one by one"""
    check("spec_k%d" % k, tmp_path, ("single",))


@pytest.mark.parametrize("k", [10, 64, 300])
def test_candidate_preparation_and_user_sum(k, tmp_path):
    check("prep_k%d" % k, tmp_path, ("tiles", "single"))


def test_device_sort_of_a_long_prefix(tmp_path):
    check("sort_k64", tmp_path, ("single",))


def test_user_group_model_with_feedback(tmp_path):
    """blocks go through process line by line, so nothing is tiled"""
    check("group_k16", tmp_path, ("single",))


def test_tiles_of_32_sections_per_wave(tmp_path):
    """k_rank_score_tile<32, .> ships but is selected only by SVDF_RANK_SECS_PER_WAVE, which is read once per process: a fresh child process runs
    positions and top 10 on streams with full tiles of 32 sections at k = 64"""
    want = {}
    for name in rr.NSEC32_CASES:
        want[name] = checker(rr.case(name), rr.case(name).write_model(str(tmp_path / (name + ".model"))))
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SVDF_RANK_SECS_PER_WAVE="32", PYTHONPATH=os.pathsep.join([os.path.dirname(tests), tests, os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, os.path.join(tests, "rank_rounding.py"), str(tmp_path)], env=env, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    for name in rr.NSEC32_CASES:
        got = rr.case(name).per_output(np.load(str(tmp_path / (name + ".npy"))))
        w, sel = want[name]
        assert got.shape == w.shape
        assert int(((got != w).any(1) & sel).sum()) == 0, name

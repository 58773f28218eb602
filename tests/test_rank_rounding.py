"""The inputs of tests/test_gpu_ranker_rounding.py have the power that file relies on (CPU only).  For every case of rank_rounding.CASES:
the numpy float32 restatement of the arithmetic contract equals the pinned port's ranker -- and the compiled reference's where it
is present -- on every compared output; every decoy that can differ at the case's width changes at least 5 compared outputs; at least 60 % of
the outputs are compared.  An output is a position, or a section's prefix in top_k mode; it is compared when it is untied in the pinned scores.

The ranker tests on random or trained models cannot see a rounding order: on 2 000 random candidates, 40 sections of 3 positives, k = 64 and
128, a sequential sum, the pairing (a0 + a1) + (a2 + a3) and a fused multiply-add each changed 0 of 120 positions.

Measured when the cases were fixed (mismatches of the restatement against port and reference: 0 everywhere); columns = outputs a decoy changes:

case             compared   sequential     pair01    serial4        fma      eight fused_prep fused_user
pos_k3            159/200            -          -          -         12          -          -          -
pos_k5            163/200            9          9          9          6          -          -          -
pos_k8            160/200           13          9          9         14          -          -          -
pos_k12           166/200           20          9          9         16         16          -          -
pos_k34           151/200           31         10          9         27         24          -          -
pos_k64           178/200           45          7          8         27         32          -          -
pos_k130          153/200           66         10          9         46         44          -          -
pos_k300          160/200           80         14         13         46         72          -          -
top10_k12          75/92            17          9          7         27         20          -          -
top40_k12          69/92            16         17          9         23         15          -          -
many_k12          187/210           20         12          7         22         17          -          -
bans_k12          167/200           20          9          9         17         16          -          -
spec_k12          556/600           40         11         17         24         35          -          -
top10_k64          72/92            36          6          8         24         21          -          -
top40_k64          70/92            21         16         10         25         30          -          -
many_k64          182/210           45          8         11         31         38          -          -
bans_k64          181/200           45          7          8         24         31          -          -
spec_k64          531/600           84         16         13         35         48          -          -
top10_k300         68/92            41          7          8         18         20          -          -
top40_k300         62/92            48         12         10         32         49          -          -
many_k300         164/210           81         18         16         52         73          -          -
bans_k300         161/200           77         13         12         43         69          -          -
spec_k300         534/600          160         16         10         65        104          -          -
prep_k10          230/320           25         10         16         15          -         24         10
prep_k64          233/320           88         18         16         50         54         52         31
prep_k300         246/320          129         17         16         65         95         64         47
top10_bans_k64     67/92            51         13         19         33         27          -          -
top10_long_k64     50/74            31          9          9         19         29          -          -
sort_k64           79/100           43          8          5         27         24          -          -
group_k16         148/200           28         16         15         29         36         23         26

Without a full chunk (k = 3) every summation order is the tail's, eight chains equal four up to two chunks, and a fused axpy shows only where
the products round (builder b), hence the dashes."""
import numpy as np
import pytest

import rank_rounding as rr
from oracle import oracle


@pytest.mark.parametrize("name", list(rr.CASES))
def test_rounding_inputs_have_power(name, tmp_path):
    c = rr.case(name)
    path = c.write_model(str(tmp_path / "m.model"))
    pinned = c.scores()
    want, compared = c.per_output(c.results(pinned)), c.compared(pinned)
    assert compared.mean() >= 0.6, (int(compared.sum()), len(compared))
    for kind in ("port", "reference") if oracle.have_reference() else ("port",):
        got, _ = c.run(lambda f: oracle.OracleRanker(kind, f, 0), path)
        got = c.per_output(got)
        assert got.shape == want.shape
        assert int((got != want).any(1)[compared].sum()) == 0, kind
    for decoy in c.decoys():
        changed = int((c.per_output(c.results(c.scores(decoy))) != want).any(1)[compared].sum())
        assert changed >= 5, (decoy, changed)


def test_one_process_call_per_line_equals_the_bulk_call(tmp_path):
    """the helper's two ways through a ranker give one answer on the port"""
    c = rr.case("pos_k12")
    path = c.write_model(str(tmp_path / "m.model"))
    a, _ = c.run(lambda f: oracle.OracleRanker("port", f, 0), path, how="rows")
    b, _ = c.run(lambda f: oracle.OracleRanker("port", f, 0), path, how="lines")
    np.testing.assert_array_equal(a, b)


def test_every_width_and_decoy_is_used():
    assert {rr.CASES[n]["k"] for n in rr.CASES if n.startswith("pos_")} == set(rr.WIDTHS)
    assert set(rr.DECOYS) == {d for n in rr.CASES for d in rr.case(n).decoys()}

"""Similar-item lists on the live model, the parts that need no GPU (svdf_item_topn, svdf_item_unit_rows): the unit-row rule
on the host against its numpy statement (tests/item_topn_rule.py), the header's pinned vectors, the decoys the GPU rounding test must tell
apart, every refusal that is decided before the device, and the list rule on a hand-made case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svdfeature_amd as sa
from item_topn_rule import DECOYS, edge_rows, pinned_case, random_rows, rule_similar, same_bits, unit_rows
from test_rank_eval import host_trainer

F32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "svdfeature_amd.h")


@pytest.mark.parametrize("k", [1, 3, 4, 7, 64, 130])
def test_unit_rows_equal_the_numpy_statement(k):
    """517 random N(0, 0.1) rows and the edge rows: zero, -0, squares that underflow, a denormal sum of squares, an overflowing one, a NaN,
    an inf -- bit for bit, NaN by position"""
    W = np.concatenate([random_rows(517, k, seed=k), edge_rows(k)])
    want = unit_rows(W)
    got = sa.item_unit_rows(W)
    assert same_bits(got, want)
    E = want[517:]
    assert not E[:3].any() and not np.signbit(E[:3]).any()             # zero, -0 and underflowing rows: +0 in every element
    assert np.isfinite(E[3]).all() and E[3].any() and np.signbit(E[3, 0])
    assert np.isnan(E[5]).all() and np.isnan(E[6, 0])
    if k > 1:
        assert not E[4].any() and np.signbit(E[4, -1]) and not E[6, 1:].any()
        # denormal squares are kept, not flushed; they carry a few bits each, so the row's length is only roughly 1
        assert 0.5 < float(np.sqrt((E[3].astype(np.float64) ** 2).sum())) < 1.5
    # the decoys of the unit rows, on the random rows: all three move bits from k = 7 on, only the reciprocal below
    changed = {d: int((unit_rows(W[:517], d).view(np.uint32) != want[:517].view(np.uint32)).sum()) for d in DECOYS}
    if k >= 7:
        assert min(changed.values()) > 0, changed
    elif k in (1, 3):                                # no full chunk: the pinned order IS index order; one square has nothing to re-round
        assert changed["reciprocal"] > 0 and changed["sequential"] == 0 and (k > 1 or changed["double"] == 0), changed


def header_vectors():
    """the PINNED VECTORS of the header: lines ` *   k = K:  in HEX ..  out HEX ..`"""
    out = []
    for line in open(HEADER):
        m = re.match(r" \*   k = (\d+):  in ((?:[0-9a-f]{8} ?)+) out ((?:[0-9a-f]{8} ?)+)$", line.rstrip("\n"))
        if m:
            vin, vout = (np.array([int(x, 16) for x in g.split()], np.uint32).view(F32) for g in m.groups()[1:])
            assert len(vin) == len(vout) == int(m.group(1))
            out.append((vin, vout))
    return out


def test_the_pinned_vectors_of_the_header_hold_on_both_statements():
    vectors = header_vectors()
    assert len(vectors) >= 5
    for vin, vout in vectors:
        assert same_bits(unit_rows(vin[None, :])[0], vout), vin
        assert same_bits(sa.item_unit_rows(vin[None, :])[0], vout), vin
    assert any(not v.any() and w.any() for w, v in vectors)        # one of them underflows to the +0 row
    assert any(np.signbit(v).any() and not v.any() for _, v in vectors)   # one overflows: -0 elements


@pytest.mark.parametrize("k", [7, 64, 130])
def test_the_rounding_inputs_tell_every_decoy_apart(k):
    """the inputs of tests/test_gpu_item_topn.py::test_rounding_is_pinned, rebuilt here: every decoy changes at least one unit-row bit and at
    least one list entry or score bit of the rule's output"""
    W = pinned_case(k)
    items = np.arange(0, len(W), 7)
    R = unit_rows(W)
    want = rule_similar(W, items, 50)
    assert not want[3].any() and (want[2] == 50).all()
    for d in DECOYS:
        assert (unit_rows(W, d).view(np.uint32) != R.view(np.uint32)).any(), d
        other = rule_similar(W, items, 50, decoy=d)
        assert (other[0] != want[0]).any() or (other[1].view(np.uint32) != want[1].view(np.uint32)).any(), d


def test_the_rule_on_a_hand_made_case():
    """six items: 1 and 2 are the same direction at different lengths (a cosine tie, broken by id; not a dot tie), 3 is a zero-norm row
    (scores 0 against everything), 4 is orthogonal to 0 with a -0 product against the +0 of item 3, 5 is the best match of 0 and banned"""
    W = np.array([[1, 0, 0, 0], [2, 2, 0, 0], [4, 4, 0, 0], [0, 0, 0, 0], [-0.0, 0, -3, 0], [8, 0, 0, 0]], F32)
    items, scores, count, nan = rule_similar(W, [0, 0, 3], 5, "cosine", [0, 1, 1, 3], [5, 3, 3])
    assert items.tolist() == [[1, 2, 3, 4, -1], [5, 1, 2, 3, 4], [0, 1, 2, 4, 5]] and count.tolist() == [4, 5, 5] and not nan.any()
    assert scores[1, 0] == 1.0 and scores[0, 0] == scores[0, 1] == F32(1) / np.sqrt(F32(2)) and not scores[2].any() and not np.signbit(scores).any()
    items, scores, count, nan = rule_similar(W, [0, 0], 5, "dot", [0, 1, 1], [5])
    assert items.tolist() == [[2, 1, 3, 4, -1], [5, 2, 1, 3, 4]] and scores[1].tolist() == [8.0, 4.0, 2.0, 0.0, 0.0]
    # a NaN row flags the sections that rank it, not the one that bans it, and not its own query's exclusion alone
    W[5, 1] = np.nan
    items, scores, count, nan = rule_similar(W, [0, 0, 5], 3, "cosine", [0, 1, 1, 1], [5])
    assert nan.tolist() == [0, 1, 1] and count.tolist() == [3, 0, 0]


def call(t, *a, **kw):
    return t.similar_items(*a, **kw)


def test_configuration_refusals_that_need_no_device(tmp_path):
    for ext in (2, 15):
        with pytest.raises(sa.SvdfError, match="item_topn: .*extend_type != 0 are not covered"):
            call(host_trainer(fmt=1, ext=ext, extra=[("num_ufeedback", 30)]), [1, 2], 5)
    with pytest.raises(sa.SvdfError, match="item_topn: common_latent_space != 0"):
        call(host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]), [1, 2], 5)
    with pytest.raises(sa.SvdfError, match="item_topn: amd:gpus > 1 is not covered"):
        call(host_trainer(extra=[("amd:gpus", 2)]), [1, 2], 5)
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    with pytest.raises(sa.SvdfError, match="item_topn: a feature_item side table changes an item's effective row .* not covered"):
        call(host_trainer(extra=[("feature_item", str(table))]), [1, 2], 5)
    with pytest.raises(sa.SvdfError, match="item_topn: call init_model / load_model and init_trainer first"):
        call(sa.Trainer(0, 0, 0, device=-2), [1, 2], 5)
    # admitted: a feature_user table, and user-group trainers of extend_type 0 / 1 -- only the device is missing
    for t in (host_trainer(extra=[("feature_user", str(table))]), host_trainer(fmt=1, extra=[("num_ufeedback", 30)]),
              host_trainer(fmt=1, ext=1, extra=[("num_ufeedback", 30)])):
        with pytest.raises(sa.SvdfError, match="item_topn needs a GPU"):
            call(t, [1, 2], 5)


def test_argument_refusals_come_before_the_device():
    t = host_trainer()
    for metric in (2, -1):
        with pytest.raises(sa.SvdfError, match="item_topn: metric must be 0 .* or 1"):
            call(t, [1, 2], 5, metric=metric)
    with pytest.raises(sa.SvdfError, match="item_topn: metric must be"):
        call(t, [1, 2], 5, metric="jaccard")
    for top_n in (0, -1, 257):
        with pytest.raises(sa.SvdfError, match="item_topn: top_n must be between 1 and 256"):
            call(t, [1, 2], top_n)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        call(t, [1, 30], 5)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        call(t, [1, 2], 5, "dot", [0, 1, 2], [3, 30])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        call(t, [1, 2], 5, "dot", [0, 1, 2], [3, 4000000000])
    with pytest.raises(sa.SvdfError, match="item_topn: ban_ptr must not decrease"):
        call(t, [1, 2], 5, "cosine", [0, 2, 1], [3, 4])
    with pytest.raises(sa.SvdfError, match="item_topn: ban_ptr must start at >= 0"):
        call(t, [1, 2], 5, "cosine", [-1, 1, 2], [3, 4])
    with pytest.raises(sa.SvdfError, match="one entry more than items"):
        call(t, [1, 2], 5, "cosine", [0, 2], [3, 4])
    # NULL outputs with sections, through the C entry point
    raw = C.CDLL(t.lib._name).svdf_item_topn          # (the declared prototype takes arrays only)
    items, out, cnt = np.array([1, 2], np.uint32), np.zeros(10, np.int32), np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for outs in ((None, ptr(cnt), ptr(cnt)), (ptr(out), None, ptr(cnt)), (ptr(out), ptr(cnt), None)):
        assert raw(C.c_void_p(t.h), C.c_long(2), ptr(items), 0, None, None, 5, outs[0], None, outs[1], outs[2]) == -1
        assert t.lib.svdf_last_error().decode() == "item_topn: bad arguments"
    assert t.counter(49) == 0


def test_a_legal_call_on_a_host_only_handle_needs_a_gpu():
    t = host_trainer()
    for metric in ("dot", "cosine", 0, 1):
        for top_n in (1, 256):
            with pytest.raises(sa.SvdfError, match="item_topn needs a GPU"):
                call(t, [1, 2, 1], top_n, metric, [0, 3, 5, 5], [7, 7, 8, 2, 5])   # duplicate bans, a query among its bans, an item twice
    with pytest.raises(sa.SvdfError, match="item_topn needs a GPU"):
        call(t, None, 40)                                                          # every item; top_n above num_item: a shorter list
    empty = call(t, np.zeros(0, np.uint32), 7)                                     # no sections: nothing to do, not even a device
    assert empty[0].shape == (0, 7) and empty[1].shape == (0, 7) and empty[2].shape == (0,) and empty[3].shape == (0,)
    assert t.counter(49) == 0 and t.counter(39) == 0

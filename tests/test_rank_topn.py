"""Top-N item lists on the live model, the parts that need no GPU: every refusal of svdf_rank_topn that is decided before the
device, on a host-only handle, and the numpy statement of the rule that tests/test_gpu_rank_topn.py compares the GPU against."""
import numpy as np
import pytest

import svdfeature_amd as sa
from rank_rounding import score_fp32
from test_rank_eval import host_trainer

F32 = np.float32


def rule_topn(U, W, bias, users, top_n, ban_ptr=None, ban_item=None, order="pinned"):
    """the documented rule: the score of DESIGN.md 6w in numpy float32 (`order`: the pinned summation order or one of rank_rounding's decoys),
    banned ids masked, higher score first and equal scores by ascending id with -0 folded onto +0; a NaN among the ranked candidates flags
    the section, whose list is then empty.  Returns (items, scores, count, nan) as Trainer.rank_topn does."""
    S, ni = len(users), len(W)
    items, scores = np.full((S, top_n), -1, np.int32), np.zeros((S, top_n), F32)
    count, nan = np.zeros(S, np.int32), np.zeros(S, np.int32)
    for s in range(S):
        sc = score_fp32(U[users[s]], W, bias, order)
        on = np.ones(ni, bool)
        if ban_ptr is not None:
            on[np.asarray(ban_item[ban_ptr[s]:ban_ptr[s + 1]], np.int64)] = False
        ids = np.flatnonzero(on)
        v = sc[ids]
        if np.isnan(v).any():
            nan[s] = 1
            continue
        v = np.where(v == 0, F32(0.0), v)               # -0 == +0
        o = np.lexsort((ids, -v))[:top_n]
        count[s] = len(o)
        items[s, :len(o)], scores[s, :len(o)] = ids[o], v[o]
    return items, scores, count, nan


def test_the_rule_on_a_hand_made_case():
    """six items whose scores are their biases (zero factor rows): a tie (items 1, 2), a ban (item 5, the best score), a +-0 pair (3, 4)"""
    W, U = np.zeros((6, 4), F32), np.ones((2, 4), F32)
    bias = np.array([1.0, 2.0, 2.0, -0.0, 0.0, 3.0], F32)
    users, ban_ptr, ban_item = [1, 0], [0, 2, 2], [5, 5]
    items, scores, count, nan = rule_topn(U, W, bias, users, 4, ban_ptr, ban_item)
    assert items.tolist() == [[1, 2, 0, 3], [5, 1, 2, 0]] and count.tolist() == [4, 4] and not nan.any()
    assert scores.tolist() == [[2.0, 2.0, 1.0, 0.0], [3.0, 2.0, 2.0, 1.0]]
    assert not np.signbit(scores).any()
    items, scores, count, nan = rule_topn(U, W, bias, users, 6, ban_ptr, ban_item)
    assert items.tolist() == [[1, 2, 0, 3, 4, -1], [5, 1, 2, 0, 3, 4]] and count.tolist() == [5, 6]
    assert scores[0, 5] == 0.0
    # a NaN flags the sections that rank it, not the one that bans it
    bias[5] = np.nan
    items, scores, count, nan = rule_topn(U, W, bias, users, 3, ban_ptr, ban_item)
    assert nan.tolist() == [0, 1] and count.tolist() == [3, 0] and items.tolist() == [[1, 2, 0], [-1, -1, -1]] and (scores[1] == 0).all()
    # ban_ptr = None: nothing is banned
    assert rule_topn(U, W, np.arange(6, dtype=F32), [0], 2)[0].tolist() == [[5, 4]]


def test_configuration_refusals_that_need_no_device(tmp_path):
    with pytest.raises(sa.SvdfError, match="rank_topn: user-group trainers"):
        host_trainer(fmt=1, extra=[("num_ufeedback", 30)]).rank_topn([1, 2], 5)
    with pytest.raises(sa.SvdfError, match="rank_topn: .*extend_type != 0"):
        host_trainer(fmt=1, ext=1, extra=[("num_ufeedback", 30)]).rank_topn([1, 2], 5)
    with pytest.raises(sa.SvdfError, match="rank_topn: common_latent_space != 0"):
        host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]).rank_topn([1, 2], 5)
    with pytest.raises(sa.SvdfError, match="rank_topn: amd:gpus > 1 is not covered"):
        host_trainer(extra=[("amd:gpus", 2)]).rank_topn([1, 2], 5)
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    for key in ("feature_user", "feature_item"):
        with pytest.raises(sa.SvdfError, match="rank_topn: .*side tables change the score"):
            host_trainer(extra=[(key, str(table))]).rank_topn([1, 2], 5)


def test_list_refusals_come_before_the_device():
    """the ranker's messages, raised while validating on the host: a host-only handle gets them, not `needs a GPU`"""
    t = host_trainer()
    with pytest.raises(sa.SvdfError, match="user feature index exceed bound"):
        t.rank_topn([1, 20], 5)
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_topn([1, 2], 5, [0, 1, 2], [3, 30])
    with pytest.raises(sa.SvdfError, match="sample item index exceed bound"):
        t.rank_topn([1, 2], 5, [0, 1, 2], [3, 4000000000])
    with pytest.raises(sa.SvdfError, match="ban_ptr must not decrease"):
        t.rank_topn([1, 2], 5, [0, 2, 1], [3, 4])
    with pytest.raises(sa.SvdfError, match="ban_ptr must start at >= 0"):
        t.rank_topn([1, 2], 5, [-1, 1, 2], [3, 4])
    with pytest.raises(sa.SvdfError, match="one entry more than users"):
        t.rank_topn([1, 2], 5, [0, 2], [3, 4])


@pytest.mark.parametrize("top_n", [0, -1, 257])
def test_top_n_out_of_bounds_names_the_bound(top_n):
    with pytest.raises(sa.SvdfError, match="top_n must be between 1 and 256.*svdf_ranker_.*top_k"):
        host_trainer().rank_topn([1, 2], top_n)


def test_a_legal_call_on_a_host_only_handle_needs_a_gpu():
    t = host_trainer()
    for top_n in (1, 256):
        with pytest.raises(sa.SvdfError, match="rank_topn needs a GPU"):
            t.rank_topn([1, 2, 1], top_n, [0, 3, 5, 5], [7, 7, 8, 5, 5])      # duplicate bans, an empty ban list, a user twice: all legal
    with pytest.raises(sa.SvdfError, match="rank_topn needs a GPU"):
        t.rank_topn([1, 2], 40)                                                 # top_n above num_item = 30: a shorter list, not a refusal
    assert t.counter(39) == 0

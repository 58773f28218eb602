"""Fold-in on the live model, the parts that need no GPU (svdf_fold_in): every refusal is decided on the host, before the
device is asked for, so a host-only handle (device=-2) answers all of them."""
import ctypes as C

import numpy as np
import pytest

import cases
import svdfeature_amd as sa
from test_rank_eval import host_trainer

LEGAL = dict(users=[1, 2, 1], ptr=[0, 2, 2, 5], item=[5, 6, 7, 7, 29], label=[1, 2, 3, 4, 5], reg=0.5)   # an empty section, an item twice, a user twice


def fold(t, write=False, **change):
    a = dict(LEGAL, **change)
    return t.fold_in(a["users"], a["ptr"], a["item"], a["label"], a["reg"], write=write)


def linked_trainer(active):
    t = sa.Trainer(0, active, 0, device=-2)
    for k, v in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=30, num_factor=8, active_type=active, base_score=0.5):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


def side_table(tmp_path):
    table = tmp_path / "feat.txt"
    table.write_text("1 3:0.5\n")
    return str(table)


CONFIGURATIONS = [
    (lambda p: linked_trainer(1), "fold_in: active_type != 0 is not covered"),
    (lambda p: host_trainer(fmt=1, extra=[("num_ufeedback", 30)]), r"fold_in: user-group trainers \(format_type = 1\) are not covered: the score has a feedback part"),
    (lambda p: host_trainer(fmt=1, ext=2, extra=[("num_ufeedback", 30)]), "fold_in: .*extend_type != 0 are not covered"),
    (lambda p: host_trainer(fmt=1, ext=15, extra=[("num_ufeedback", 30)]), "fold_in: .*extend_type != 0 are not covered"),
    (lambda p: host_trainer(nu=30, extra=[("common_latent_space", 1), ("common_feedback_space", 1)]), "fold_in: common_latent_space != 0"),
    (lambda p: host_trainer(extra=[("feature_user", side_table(p))]), "fold_in: feature_user / feature_item side tables change the score"),
    (lambda p: host_trainer(extra=[("feature_item", side_table(p))]), "fold_in: feature_user / feature_item side tables change the score"),
    (lambda p: host_trainer(extra=[("amd:gpus", 2)]), "fold_in: amd:gpus > 1 is not covered"),
    (lambda p: sa.Trainer(0, 0, 0, device=-2), "fold_in: call init_model / load_model and init_trainer first"),
    (lambda p: host_trainer(extra=[("num_factor", 129)]), "fold_in: num_factor must be at most 128"),
]


@pytest.mark.parametrize("make, message", CONFIGURATIONS)
def test_configuration_refusals_need_no_device(make, message, tmp_path):
    t = make(tmp_path)
    with pytest.raises(sa.SvdfError, match=message):
        fold(t)
    assert t.counter(62) == 0


ARGUMENTS = [
    (dict(reg=0.0), "fold_in: reg must be finite and > 0"),
    (dict(reg=-1.0), "fold_in: reg must be finite and > 0"),
    (dict(reg=float("inf")), "fold_in: reg must be finite and > 0"),
    (dict(reg=float("nan")), "fold_in: reg must be finite and > 0"),
    (dict(ptr=[0, 3, 2, 5]), "fold_in: ptr must not decrease"),
    (dict(ptr=[-1, 2, 2, 5]), "fold_in: ptr must start at >= 0"),
    (dict(ptr=[0, 2, 5]), "fold_in: ptr must have one entry more than users"),
    (dict(ptr=[0, 2, 2, 6]), "fold_in: item and label must be equally long"),
    (dict(users=[1, 20, 3]), "user feature index exceed bound"),
    (dict(item=[5, 6, 7, 7, 30]), "sample item index exceed bound"),
]


@pytest.mark.parametrize("change, message", ARGUMENTS)
def test_argument_refusals_come_before_the_device(change, message):
    t = host_trainer()
    for write in (False, True):
        with pytest.raises(sa.SvdfError, match=message):
            fold(t, write=write, **dict(dict(users=[1, 2, 3]), **change))
    assert t.counter(62) == 0


def test_null_arrays_with_sections_are_bad_arguments():
    t = host_trainer()
    raw = C.CDLL(t.lib._name).svdf_fold_in   # (the declared prototype takes arrays only)
    a = [np.array(LEGAL["users"], np.uint32), np.array(LEGAL["ptr"], np.int64), np.array(LEGAL["item"], np.uint32),
         np.array(LEGAL["label"], np.float32), np.zeros(24, np.float32)]
    for missing in range(5):
        p = [None if i == missing else x.ctypes.data_as(C.c_void_p) for i, x in enumerate(a)]
        assert raw(C.c_void_p(t.h), C.c_long(3), p[0], p[1], p[2], p[3], C.c_float(0.5), 0, p[4]) == -1
        assert t.lib.svdf_last_error().decode() == "fold_in: bad arguments"


def test_a_legal_call_needs_a_gpu_and_no_sections_need_nothing():
    t = host_trainer()
    with pytest.raises(sa.SvdfError, match="fold_in: user 1 is written by two sections"):
        fold(t, write=True)
    with pytest.raises(sa.SvdfError, match="fold_in needs a GPU"):
        fold(t, write=False)                      # a repeated user is legal when nothing is written
    for write in (False, True):
        with pytest.raises(sa.SvdfError, match="fold_in needs a GPU"):
            fold(t, write=write, users=[1, 2, 3])
        rows = t.fold_in([], [0], [], [], 1.0, write=write)
        assert rows.shape == (0, 8) and rows.dtype == np.float32
    assert t.counter(62) == 0

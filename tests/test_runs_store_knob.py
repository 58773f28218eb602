"""Knob runs_store (svdf_config.cpp): the store policy of the staged runs kernel, 0 plain, 1 the bias words nontemporal, 2 rows and bias words sc1 write-through.
Validated on the host: a host-only handle takes every legal value and refuses the others by name."""
import pytest

import cases
import svdfeature_amd as sa


def host_trainer():
    t = sa.Trainer(0, 0, 0, device=-2)
    for k, v in cases.conf_with(cases.BASICMF_CONF, num_user=20, num_item=30, num_factor=8):
        t.set_param(k, v)
    t.init_model()
    t.init_trainer()
    return t


def test_legal_values_are_taken():
    t = host_trainer()
    for v in (0, 1, 2, 0):
        t.set_knob("runs_store", v)


@pytest.mark.parametrize("value", [-1, 3, 4, 5, 10, 64, 255, 2 ** 31])
def test_values_outside_0_to_2_are_refused(value):
    t = host_trainer()
    with pytest.raises(sa.SvdfError, match="runs_store must be 0 .plain., 1 .nontemporal bias words. or 2 .sc1 write-through."):
        t.set_knob("runs_store", value)
    t.set_knob("runs_store", 2)   # the handle stays usable

"""Point attribute maps, picking and lifting on the host emulator (tools/emu: k_ray_attributes / k_lift_to_points of csrc/pointmaps.hip compiled
for the host, the unchanged render kernels in front of them) against the float64 restatements of tests/pointmaps_case.py.  The kernel cases run
at their smallest sizes (SR*K below, across and a few times 64; every C of both sum instances at one of them); through the model only small_k4
runs here -- the device suite (tests/test_gpu_pointmaps.py) carries every size, small_k8, the cut route, per-point frames and the module.
Without the feature the entry points do not exist: every test here fails."""
import pytest
import torch

import pointmaps_case as PM
from emu_util import emu_backend


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("SR,K", PM.EMU_SHAPES)
def test_emulated_ray_attributes_against_float64(SR, K):
    PM.check_ray_attributes(SR, K, "cpu", cs=PM.CS if (SR, K) == (16, 8) else (0, 3, 5, 70))


@pytest.mark.parametrize("SR,K", PM.EMU_SHAPES)
def test_emulated_lift_against_float64(SR, K):
    PM.check_lift(SR, K, "cpu", cs=PM.LIFT_CS if (SR, K) == (16, 8) else (0, 3))


@pytest.mark.parametrize("SR,K", [(16, 3), (65, 12)])
def test_emulated_adjoint(SR, K):
    PM.check_adjoint(SR, K, "cpu")


def test_emulated_entry_point_refusals():
    PM.check_entry_refusals("cpu")


def test_emulated_model_against_the_oracle():
    PM.check_model("small_k4", 600.0, "cpu")

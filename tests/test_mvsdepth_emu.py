"""Depth maps from images on the host emulator (tools/emu: k_channels_last / k_cost_volume / k_depth_regress / k_depth_to_points of
csrc/mvsdepth.hip compiled for the host) through the unchanged Python of pointnerf_amd/ops.py: the checks of tests/mvsdepth_case.py against
the float64 restatements and the reference fixture (tests/golden/refmvsdepth.npz), with the bars the fixture records.  The networks and the
model shell run on the device suite (tests/test_gpu_mvsdepth.py).  Without the feature neither the functions nor the symbols exist: every
test here fails."""
import pytest
import torch

import mvsdepth_case as MC
from emu_util import emu_backend


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("name", list(MC.CV_CASES))
def test_emulated_cost_volume(emu, name):
    MC.check_cost_volume(name, "cpu")


@pytest.mark.parametrize("name", list(MC.RG_CASES))
def test_emulated_depth_regression(emu, name):
    MC.check_regress(name, "cpu")


def test_emulated_nan_logit_gives_nan_depth(emu):
    MC.check_regress_nan("cpu")


@pytest.mark.parametrize("name", list(MC.DP_CASES))
def test_emulated_depth_to_points(emu, name):
    MC.check_points(name, "cpu")


def test_emulated_entry_point_errors(emu):
    MC.check_entry_point_errors("cpu")


def test_cpu_tensors_are_refused_without_the_emulator():
    MC.check_cpu_tensors_refused()


def test_fixture_holds_numbers_and_names_only():
    """numeric arrays and two lists of names; every margin recorded; under the size limit for a committed file"""
    import os
    fx = MC.fixture()
    assert os.path.getsize(MC.FIX) < 1000000
    assert all(v.dtype.kind in "fiuU" for v in fx.values()), {k: v.dtype for k, v in fx.items() if v.dtype.kind not in "fiuU"}
    assert sorted(k for k, v in fx.items() if v.dtype.kind == "U") == ["mvsnet_keys", "pyr_keys"]
    assert all(float(fx[k]) > 0 for k in fx if k.startswith("dev_")) and sum(k.startswith("dev_") for k in fx) == 18

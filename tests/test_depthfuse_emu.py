"""Depth-map fusion on the host emulator (tools/emu: k_geo_consistency / k_fuse_flag / k_fuse_write / k_alpha_hull of csrc/depthfuse.hip
compiled for the host) through the unchanged Python of pointnerf_amd/point_init.py: the checks of tests/depthfuse_case.py against the
float64 restatement, the torch restatement of the selection and the reference fixture (tests/golden/refdepthfuse.npz).  Every case but the
96 x 128 one runs here (the device suite carries it, and the chain into the voxel down-sampling, whose host code asks for a device tensor).
Without the feature neither the functions nor the symbols exist: every test here fails."""
import pytest
import torch

import depthfuse_case as DC
from emu_util import emu_backend


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("key", ["v1", "v2", "v5"])
def test_emulated_threshold_decisions_and_depth_avg(emu, key):
    DC.check_thresholds(key, "cpu")


@pytest.mark.parametrize("name", DC.LIST_CASES)
def test_emulated_selection_and_order(emu, name):
    DC.check_selection(name, "cpu")


def test_emulated_lists_against_the_reference_fixture(emu):
    DC.check_fixture_end_to_end("cpu")


def test_emulated_hull(emu):
    DC.check_hull("cpu")


def test_emulated_refusals_and_entry_point_errors(emu):
    DC.check_refusals("cpu")


def test_emulated_reproducible_and_front_door(emu):
    DC.check_reproducible("cpu")


def test_cpu_tensors_are_refused_without_the_emulator():
    DC.check_cpu_tensors_refused()

"""Points from an external cloud on the host emulator (tools/emu: k_nearest_view / k_occ_set / k_occ_test / k_crop_flag / k_take_rows /
k_group_rank / k_group_place / k_group_offsets of csrc/cloudinit.hip compiled for the host) through the unchanged Python of
pointnerf_amd/point_init.py: the checks of tests/cloudinit_case.py against the float64 restatement, torch's own indexing and sorting and the
reference fixture (tests/golden/refcloudinit.npz).  Every case runs here but the chain into the voxel down-sampling, whose host code asks
for a device tensor (the device suite carries it).  Without the feature neither the functions nor the symbols exist: every test here fails."""
import pytest
import torch

import cloudinit_case as CC
from emu_util import emu_backend


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("name", list(CC.NV_CASES))
def test_emulated_nearest_view_against_float64(emu, name):
    CC.check_nearest(name, "cpu")


def test_emulated_occupancy_merge(emu):
    CC.check_merge("cpu")


def test_emulated_crop(emu):
    CC.check_crop("cpu")


@pytest.mark.parametrize("name", list(CC.GROUP_CASES))
def test_emulated_grouping(emu, name):
    CC.check_group(name, "cpu")


def test_emulated_end_to_end_against_the_reference_fixture(emu):
    CC.check_end_to_end("cpu")


def test_emulated_neural_points_plumbing(emu):
    CC.check_neural_points("cpu")


def test_emulated_reproducible(emu):
    CC.check_reproducible("cpu")


def test_emulated_refusals_and_entry_point_errors(emu):
    CC.check_refusals("cpu")


def test_cpu_tensors_are_refused_without_the_emulator():
    CC.check_cpu_tensors_refused()

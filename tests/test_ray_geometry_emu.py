"""Per-ray depth and opacity maps of render-only passes on the host emulator (tools/emu: k_ray_geometry / k_geometry_canvas of csrc/raygeom.hip
compiled for the host, the unchanged render kernels in front of them) against the float64 restatement of tests/geometry_case.py.  The two new
kernels run at every size of the device tests (tests/test_gpu_ray_geometry.py); through the model only small_k4 runs here -- an emulated
render of the larger cases takes half a minute and more, and the device suite carries them all (small_k8, the cut route, per-point frames,
the unchanged outputs, render_image).  Without the feature the entry points and the attribute do not exist: every test here fails."""
import pytest
import torch

import geometry_case as G
from emu_util import emu_backend


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("SR", G.KERNEL_SR)
def test_emulated_kernel_against_float64(SR):
    G.check_kernel(SR, "cpu")


@pytest.mark.parametrize("SR", G.KERNEL_SR)
def test_emulated_kernel_where_no_ray_crosses(SR):
    G.check_kernel(SR, "cpu", sigma_scale=0.02)


def test_emulated_entry_point_refusals():
    G.check_entry_refusals("cpu")


@pytest.mark.parametrize("shift", [0.0, 150.0, 600.0])
def test_emulated_forward_against_the_oracle(shift):
    G.check_model("small_k4", shift, "cpu")


def test_emulated_refusals_name_the_option():
    G.check_refusals("cpu")


def test_emulated_geometry_canvas():
    G.check_canvas("cpu")

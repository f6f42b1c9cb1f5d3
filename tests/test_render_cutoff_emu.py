"""Early ray termination of render-only passes on the host emulator (tools/emu: k_cut_stage / k_cut_totals and the staged driver compiled for
the host, the unchanged aggregator and colour kernels behind them) against the torch-CPU restatement of tests/cutoff_case.py, at the sizes
of the device tests (tests/test_gpu_render_cutoff.py).  Without the feature the attributes, the keywords and the entry points do not exist."""
import pytest
import torch

import cutoff_case as C
from emu_util import emu_backend


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("name,shift,c,B", C.ROWS)
def test_emulated_cut_render_matches_the_restatement(name, shift, c, B):
    _, ref = C.check_row(name, shift, c, B, "cpu")
    C.check_terminates(ref, 4)


def test_emulated_bitwise_identities():
    C.check_bitwise_identities("small_k4", 600.0, "cpu")


@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_emulated_cut_render_where_nothing_terminates(name):
    C.check_no_termination(name, "cpu")


def test_emulated_cut_render_with_per_point_frames():
    C.check_frames("cpu")


def test_emulated_refusals_name_the_option():
    C.check_refusals("cpu")


def test_emulated_render_image_with_a_cutoff():
    C.check_render_image("cpu")


def test_emulated_cut_render_with_two_products():
    C.check_arithmetic_option("cpu", "products2")


def test_emulated_entry_point_arguments():
    C.check_entry_point_arguments("cpu")


@pytest.mark.parametrize("SR", [16, 80, 128])
@pytest.mark.parametrize("B", [1, 5, 16, 64, 100])
def test_emulated_cut_stage_on_synthetic_arrays(SR, B):
    C.check_cut_stage(SR, B, "cpu")

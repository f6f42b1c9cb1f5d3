"""Early ray termination of render-only passes on the device: pnerf_render_forward_cut / pnerf_cut_stage (csrc/render.hip: k_cut_stage,
k_cut_totals, the staged driver over the unchanged aggregator and colour kernels) against the torch-CPU restatement of tests/cutoff_case.py.
Shapes: small_k4 (100 rays, SR 16, K 4) and small_k8 (144 rays, SR 24, K 8) made opaque by a shift of alpha_branch.0.bias; the stage step alone on
37 rays x SR 16 / 80 / 128 (one, two and exactly two 64-slot wave chunks) with stages of 1 / 5 / 16 / 64 / 100 slots.  Bars: the forward bar 1e-4
(sigma relatively), the analytic bound 1.002 c + 1e-4 against the full render, exact equality where the launches are the same."""
import pytest

import cutoff_case as C
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,shift,c,B", C.ROWS)
def test_cut_render_matches_the_restatement(name, shift, c, B):
    _, ref = C.check_row(name, shift, c, B, DEV)
    C.check_terminates(ref, 4)


@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_bitwise_identities(name):
    C.check_bitwise_identities(name, 600.0, DEV)


@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_cut_render_where_nothing_terminates(name):
    C.check_no_termination(name, DEV)


def test_cut_render_with_per_point_frames():
    C.check_frames(DEV)


def test_refusals_name_the_option():
    C.check_refusals(DEV)


def test_render_image_with_a_cutoff():
    C.check_render_image(DEV)


@pytest.mark.parametrize("option", ["products2", "e4m3"])
def test_cut_render_under_the_other_inference_arithmetics(option):
    C.check_arithmetic_option(DEV, option)


def test_entry_point_arguments():
    C.check_entry_point_arguments(DEV)


@pytest.mark.parametrize("SR", [16, 80, 128])
@pytest.mark.parametrize("B", [1, 5, 16, 64, 100])
def test_cut_stage_on_synthetic_arrays(SR, B):
    C.check_cut_stage(SR, B, DEV)

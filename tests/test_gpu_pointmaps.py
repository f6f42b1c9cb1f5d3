"""Point attribute maps, picking and lifting on the device: pnerf_ray_attributes / pnerf_lift_to_points (csrc/pointmaps.hip) and
pointnerf_amd/point_maps.py against the float64 restatements of tests/pointmaps_case.py.  Shapes: the kernels alone on 37 rays x 500 points at
SR 1 / 16 / 65 / 128 x K 1 / 3 / 8 / 12 / 16 (SR*K below, across and many times the 64 entries of a wave chunk), C 0 / 1 / 3 / 4 (the
entry-parallel instance) / 5 / 32 / 33 / 64 / 70 (the column-parallel one, the 64-column pass boundary), lifting at C 0 / 1 / 3 / 8; through the
model on small_k4 (100 rays, SR 16, K 4) and small_k8 (144 rays, SR 24, K 8) at alpha-bias shifts 0 / 150 / 600; a 24 x 24 image in three
chunks.  Bars (derived in pointmaps_case.py): (SR*K + 2) 2^-24 A for the sums, bit equality for the pick, (n_p + 3) 2^-24 A_p for the lift,
the forward bar 1e-4 through the model."""
import pytest

import pointmaps_case as PM
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", PM.KS)
@pytest.mark.parametrize("SR", PM.SRS)
def test_ray_attributes_against_float64(SR, K):
    PM.check_ray_attributes(SR, K, DEV)


@pytest.mark.parametrize("K", PM.KS)
@pytest.mark.parametrize("SR", PM.SRS)
def test_lift_against_float64(SR, K):
    PM.check_lift(SR, K, DEV)


@pytest.mark.parametrize("K", PM.KS)
@pytest.mark.parametrize("SR", PM.SRS)
def test_adjoint(SR, K):
    PM.check_adjoint(SR, K, DEV)


def test_entry_point_refusals():
    PM.check_entry_refusals(DEV)


@pytest.mark.parametrize("shift", [0.0, 150.0, 600.0])
@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_model_against_the_oracle(name, shift):
    PM.check_model(name, shift, DEV)


def test_cut_route():
    PM.check_cut_route(DEV)


def test_per_point_frames():
    PM.check_frames(DEV)


def test_module_functions_on_an_image():
    PM.check_module(DEV)

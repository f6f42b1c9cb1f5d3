"""Points from an external cloud on the device (csrc/cloudinit.hip through pointnerf_amd/point_init.py): the nearest view against the
float64 restatement on decided points, merge / crop / grouping exactly, the whole route against the reference fixture, the chain into the
voxel down-sampling, the per-view embedding plumbing, refusals and reproducibility (tests/cloudinit_case.py).  The largest inputs are 5 000
points x 24 cameras, 513 points x 549 cameras and 70 000 indices to group."""
import pytest

import cloudinit_case as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(CC.NV_CASES))
def test_nearest_view_against_float64(name):
    CC.check_nearest(name, DEV)


def test_occupancy_merge():
    CC.check_merge(DEV)


def test_crop():
    CC.check_crop(DEV)


@pytest.mark.parametrize("name", list(CC.GROUP_CASES))
def test_grouping(name):
    CC.check_group(name, DEV)


def test_end_to_end_against_the_reference_fixture():
    CC.check_end_to_end(DEV)


def test_vox_chain():
    CC.check_vox_chain(DEV)


def test_neural_points_plumbing():
    CC.check_neural_points(DEV)


def test_reproducible():
    CC.check_reproducible(DEV)


def test_refusals_and_entry_point_errors():
    CC.check_refusals(DEV)
    CC.check_cpu_tensors_refused()

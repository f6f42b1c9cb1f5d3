"""Depth-map fusion on the device (csrc/depthfuse.hip through pointnerf_amd/point_init.py): threshold decisions and depth_avg against the
float64 restatement on decided pairs, selection and order against the torch restatement of the reference's lines, the returned lists against
the reference fixture, the visual hull, refusals, reproducibility and the chain into the voxel down-sampling (tests/depthfuse_case.py).
The largest input is 6 views of 96 x 128."""
import pytest

import depthfuse_case as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("key", ["v1", "v2", "v5", "v6"])
def test_threshold_decisions_and_depth_avg(key):
    DC.check_thresholds(key, DEV)


@pytest.mark.parametrize("name", list(DC.VARIANTS))
def test_selection_and_order(name):
    DC.check_selection(name, DEV)


def test_lists_against_the_reference_fixture():
    DC.check_fixture_end_to_end(DEV)


def test_hull():
    DC.check_hull(DEV)


def test_refusals_and_entry_point_errors():
    DC.check_refusals(DEV)
    DC.check_cpu_tensors_refused()


def test_reproducible_and_front_door():
    DC.check_reproducible(DEV)


def test_vox_chain():
    DC.check_vox_chain(DEV)

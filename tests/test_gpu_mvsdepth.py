"""Depth maps from images on the device (csrc/mvsdepth.hip through pointnerf_amd/ops.py, depth_estimators.py, mvs_points_model.py, the
mode-1 model shell and point_init): the three kernels against their float64 restatements and the reference fixture, MVSNet.forward end to
end, the feature pyramid, the checkpoint key lists, create_model(mode=1) from a get_init_item dictionary to filter_by_masks_gpu and
query_embedding, the plain-tensor front door, refusals and reproducibility (tests/mvsdepth_case.py).  The largest input is three 64 x 96
images at 16 depth planes.  Without the feature the entry points do not exist and the shell raises: every test here fails."""
import pytest

import mvsdepth_case as MC
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(MC.CV_CASES))
def test_cost_volume_against_float64_and_the_reference(name):
    MC.check_cost_volume(name, DEV)


@pytest.mark.parametrize("name", list(MC.RG_CASES))
def test_depth_regression_against_float64_and_the_reference(name):
    MC.check_regress(name, DEV)


def test_nan_logit_gives_nan_depth():
    MC.check_regress_nan(DEV)


@pytest.mark.parametrize("name", list(MC.DP_CASES))
def test_depth_to_points_indices_mask_and_positions(name):
    MC.check_points(name, DEV)


def test_entry_point_errors():
    MC.check_entry_point_errors(DEV)


def test_cpu_tensors_are_refused():
    MC.check_cpu_tensors_refused()


def test_mvsnet_forward_end_to_end():
    MC.check_e2e(DEV)


def test_feature_pyramid():
    MC.check_pyramid(DEV)


def test_reference_key_lists_load_strictly(tmp_path):
    MC.check_state_dicts(DEV, tmp_path)


def test_mode_1_shell_from_init_item_to_query_embedding():
    MC.check_shell(DEV)


def test_points_from_images_is_the_chain_by_hand():
    MC.check_front_door(DEV)


def test_refusals_name_their_option():
    MC.check_refusals(DEV)

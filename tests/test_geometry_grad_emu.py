"""Host-emulator twin of tests/test_gpu_geometry_grad.py (tests/geometry_grad_case.py): the real GEOM instance of k_raymarch_backward and the
two kernels of the geometry loss pass, built for x86, against float64 -- the cases, bars and bit conditions of the device tests.  The
emulator's expf is the host's libm; the order of every wave scan and sum is the device's.  What needs the aggregator on the device (the model,
the chunked recompute, the shell) is in the device file only; the shell's refusals and the option's plumbing are checked here."""
import types

import pytest
import torch

import geometry_grad_case as G
import raymarch_case as RC
from emu_util import emu_backend

_runs = {}
CASE_VARIANTS = [(c, v) for c in RC.CASES for v in G.VARIANTS]
_id = lambda cv: "%s-%s" % (RC.case_id(cv[0]), cv[1])


@pytest.fixture(autouse=True)
def _emu():
    with emu_backend():
        yield


def _run(case, variant):
    key = (case, variant)
    if key not in _runs:
        _runs[key] = G.hip_backward_geom(G.reference(case, variant), "cpu")
    return _runs[key]


@pytest.mark.parametrize("cv", CASE_VARIANTS, ids=_id)
def test_emulated_geometry_backward_per_ray_against_float64(cv):
    G.check_backward(G.reference(*cv), _run(*cv))


@pytest.mark.parametrize("cv", CASE_VARIANTS, ids=_id)
def test_emulated_rgb_gradient_unchanged_and_invalid_slots(cv):
    G.check_rgb_unchanged_and_invalid_slots(G.reference(*cv), _run(*cv), "cpu")


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_emulated_zero_geometry_gradient_is_the_existing_backward(case):
    G.check_zero_geom_is_plain(G.reference(case, "both"), "cpu")


@pytest.mark.parametrize("SR", (1, 65, 130))
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_emulated_gradient_scales_by_exact_powers_of_two(SR, variant):
    G.check_scaling(G.reference(("thin", SR, "white"), variant), "cpu")


@pytest.mark.parametrize("case", [("thin", 65, "white"), ("opaque", 65, "white"), ("mixed", 130, "none")], ids=RC.case_id)
def test_emulated_ray_alone_guarded_memory_and_poisoned_depths(case):
    ref = G.reference(case, "both")
    grad = _run(case, "both")
    for r in (0, ref.base.rows["surface"][-1], RC.R - 1):
        G.check_ray_alone(ref, grad, "cpu", r)
    G.check_guarded_memory(ref, grad, "cpu")
    G.check_poisoned_z(ref, grad, "cpu")


def test_emulated_return_codes():
    G.check_return_codes("cpu")
    G.check_render_backward_geom_return_codes("cpu")


@pytest.mark.parametrize("mask_kind", G.MASKS)
def test_emulated_loss_pass_against_float64(mask_kind):
    G.check_loss_pass(mask_kind, "cpu")


def test_shell_accepts_the_two_items_and_refuses_the_rest():
    """check_setup_loss: coarse_depth / coarse_is_background are accepted with their weights; any other item name raises, naming it"""
    from pointnerf_amd.mvs_points_volumetric_model import MvsPointsVolumetricModel
    mk = lambda **kw: types.SimpleNamespace(color_loss_items=None, sparse_loss_weight=0, **kw)
    m = MvsPointsVolumetricModel()
    opt = mk(depth_loss_items="coarse_depth", depth_loss_weights=[0.1], bg_loss_items=["coarse_is_background"], bg_loss_weights=[0.5])
    m.check_setup_loss(opt)
    assert opt.depth_loss_items == ["coarse_depth"] and opt.depth_loss_weights == [0.1] and opt.bg_loss_weights == [0.5]
    assert m.loss_names == ["total", "coarse_raycolor", "coarse_depth", "coarse_is_background"]
    with pytest.raises(NotImplementedError, match="fine_depth"):
        m.check_setup_loss(mk(depth_loss_items=["coarse_depth", "fine_depth"]))
    with pytest.raises(NotImplementedError, match="coarse_mask"):
        m.check_setup_loss(mk(bg_loss_items=["coarse_mask"]))
    m.check_setup_loss(mk())                                        # no item: the names it had
    assert m.loss_names == ["total", "coarse_raycolor"]


def test_losses_need_the_differentiable_geometry_and_hot_path_loss_refuses_the_items():
    from pointnerf_amd import dist as pdist, losses
    with pytest.raises(RuntimeError, match="geometry_grad"):
        losses.depth({}, torch.zeros(1, 3, 1), torch.zeros(1, 3, 1))
    with pytest.raises(RuntimeError, match="geometry_grad"):
        losses.background({"_dense_geometry": {"depth": None}}, torch.zeros(1, 3, 1))      # the render-only maps are not the differentiable form
    opt = types.SimpleNamespace(depth_loss_items=["coarse_depth"], bg_loss_items=[], zero_one_loss_items=[])
    with pytest.raises(NotImplementedError, match="depth_loss_items"):
        pdist.hot_path_loss(opt, {}, None)


def test_option_defaults_off_and_names_itself_in_refusals():
    from pointnerf_amd import config
    from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
    opt = config.lego_opt()
    model = NeuralPointsRayMarching(opt=opt)
    assert model.geometry_grad is False and model._geometry_grad_setting() is False
    opt.geometry_grad = True
    try:
        model = NeuralPointsRayMarching(opt=opt)
    finally:
        del opt.geometry_grad
    assert model.geometry_grad is True
    model.neural_points = types.SimpleNamespace(Rw2c=torch.eye(3))
    assert model._geometry_grad_setting() is True
    model.transmittance_cutoff = 0.1
    with pytest.raises(NotImplementedError, match="geometry_grad"):
        model._geometry_grad_setting()
    model.transmittance_cutoff = 0.0
    model.neural_points = types.SimpleNamespace(Rw2c=torch.eye(3)[None].repeat(4, 1, 1))
    with pytest.raises(NotImplementedError, match="geometry_grad"):
        model._geometry_grad_setting()
    model.neural_points = types.SimpleNamespace(Rw2c=torch.eye(3))
    model.fused_probe = True
    with pytest.raises(NotImplementedError, match="geometry_grad"):
        model._geometry_grad_setting()

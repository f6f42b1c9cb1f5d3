"""Per-ray depth and opacity maps of render-only passes on the device: pnerf_ray_geometry / pnerf_geometry_canvas (csrc/raygeom.hip) against
the float64 restatement of tests/geometry_case.py.  Shapes: the kernel alone on 37 rays x SR 16 / 24 / 64 / 65 / 80 / 128 (one 64-slot wave
chunk, the chunk boundary, a partial second chunk, two full chunks); through the model on small_k4 (100 rays, SR 16, K 4) and small_k8 (144
rays, SR 24, K 8) at alpha-bias shifts 0 / 150 / 600; a 24 x 24 image in three chunks.  Bars: 1e-5 for the kernel's fp32 sums against float64
on the same inputs, the forward bar 1e-4 through the model, 1e-6 / bit equality for the median depth off the near rays."""
import pytest

import geometry_case as G
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("SR", G.KERNEL_SR)
def test_kernel_against_float64(SR):
    G.check_kernel(SR, DEV)


@pytest.mark.parametrize("SR", G.KERNEL_SR)
def test_kernel_where_no_ray_crosses(SR):
    G.check_kernel(SR, DEV, sigma_scale=0.02)


def test_entry_point_refusals():
    G.check_entry_refusals(DEV)


@pytest.mark.parametrize("shift", [0.0, 150.0, 600.0])
@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_forward_against_the_oracle(name, shift):
    G.check_model(name, shift, DEV)


@pytest.mark.parametrize("name", ["small_k4", "small_k8"])
def test_outputs_are_unchanged_with_the_attribute_off(name):
    G.check_unchanged(name, 600.0, DEV)


def test_cut_route():
    G.check_cut_route(DEV)


def test_per_point_frames():
    G.check_frames(DEV)


def test_refusals_name_the_option():
    G.check_refusals(DEV)


def test_render_image_with_geometry():
    G.check_render_image(DEV)


@pytest.mark.parametrize("h,w", [(24, 24), (5, 9)])
def test_geometry_canvas(h, w):
    G.check_canvas(DEV, h, w)


def test_test_views_with_geometry(tmp_path):
    """eval_loop.test_views(geometry=True) through the model shell on two views of 24 x 32 rays in chunks of 500: the three canvases handed to
    on_view are the marcher's own maps of the view's rays scattered by pixel (bit for bit: the same kernels), every returned score keeps its
    value, the attribute is restored."""
    import numpy as np
    import torch
    from test_gpu_model_shell import _scene
    from oracle import pyref
    from pointnerf_amd import eval_loop, scenes
    from pointnerf_amd.neural_points_volumetric_model import fill_invalid
    H, W = 24, 32
    opt, m, *_ = _scene("small_k8", tmp_path, is_train=0)
    views = []
    for i, theta in enumerate((30.0, 95.0)):
        c2w, intr = scenes.synth_camera(theta)
        py, px = np.meshgrid(np.arange(388, 388 + H), np.arange(404, 404 + W), indexing="ij")   # (half of the block looks past the cloud)
        inp = scenes.ray_dict(c2w, intr, px, py, gt_seed=i)
        inp["pixel_idx"] = inp["pixel_idx"] - np.array([404, 388], np.float32)          # the view's own H x W pixel grid, row-major
        views.append(dict(pyref.to_torch_inputs(inp), id=i))
    seen = []
    psnr0, avg0 = eval_loop.test_views(m, views, opt, H, W, chunk=500, on_view=lambda i, v: seen.append(sorted(v)))
    got = []
    psnr1, avg1 = eval_loop.test_views(m, views, opt, H, W, chunk=500, geometry=True, on_view=lambda i, v: got.append({k: t.clone() for k, t in v.items()}))
    assert psnr1 == psnr0 and avg1 == avg0
    marcher = m.net_ray_marching
    assert marcher.ray_geometry is False
    keys = ("coarse_depth", "coarse_median_depth", "coarse_acc")
    assert len(got) == 2 and sorted(got[0]) == sorted(seen[0] + list(keys))
    for view, vis in zip(views, got):
        d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in view.items() if k != "id"}
        marcher.ray_geometry = True
        try:
            with torch.no_grad():
                out = marcher(**d)
        finally:
            marcher.ray_geometry = False
        full = fill_invalid(out, d["bg_color"])
        hit = out["ray_mask"][0] > 0
        assert 50 < int(hit.sum()) < H * W
        for k in keys:
            assert tuple(vis[k].shape) == (H, W) and torch.equal(vis[k].reshape(-1), full[k][0, :, 0]), k      # (the rays are the row-major pixel grid)
        acc, depth = vis["coarse_acc"].reshape(-1), vis["coarse_depth"].reshape(-1)
        assert float(acc[~hit].abs().sum()) == 0.0 and float(depth[~hit].abs().sum()) == 0.0                   # 0 where the ray missed
        assert float(acc[hit].max()) > 1e-4 and float(acc.min()) >= 0.0 and float(acc.max()) <= 1.0 + 1e-6
        assert float(depth[hit].max()) > 2.0 and float(depth.max()) <= 6.0                                     # samples lie between near = 2 and far = 6

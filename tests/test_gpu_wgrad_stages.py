"""The weight-gradient GEMMs (k_wgrad_f16, k_wgrad_x0) at the edges of their stage rings, through the render entry points: a workgroup walks
stages of 32 rows (one plane) or 16 rows (two planes) of the saved k-major planes through a ring of four LDS slots, stage i of workgroup b being
stage b + grid x i of the call.  The colour layers' rows are the valid samples, the aggregator layers' the samples' neighbour rows in 64-row
tiles per sample class, so both are steered by the number of valid samples (tests/color_tiles_case.py: by choosing rays) and, for the grid --
which the host sizes from the CAPACITY it was given, not from the device's count -- by a capacity above the count:
  fewer stages than ring slots   40 samples: one colour tile = 2 stages of 32 rows; 8 samples: one or two aggregator tiles
  exactly a ring                 128 samples (one plane: 4 x 32 rows), 64 samples (two planes: 4 x 16 rows)
  one stage past the grid        128 samples in a capacity of 400 .. 450 (one plane: 3 colour workgroups, 4 stages), 256 samples in a capacity
                                 of 320 .. 360 (two planes: 5 colour workgroups, 16 stages); the aggregator layers' grids are the capacity's tiles,
                                 so the same calls leave some of their workgroups without a stage and give others a second one
Reference: the oracle's autograd at the bars of tests/test_gpu_backward.py (_check: every MLP tensor within 5e-4 of its largest element), in both
plane modes.  (Nothing outside the library can read the saved planes, so a float64 product of the planes themselves is not available to a
test.)"""
import numpy as np
import pytest
import torch

import test_gpu_backward as TB
from color_tiles_case import forced_case
from gpu_util import DEV
from pointnerf_amd import ops
from pointnerf_amd.point_query import lighting_fast_querier

pytestmark = pytest.mark.gpu
# (valid samples, capacity handed to the entry points)
CALLS = [(8, 8), (40, 40), (64, 64), (128, 128), (128, 400), (128, 450), (256, 256), (256, 320), (256, 360), (1000, 1000), (1000, 1237)]
_oracle = {}


def _grads(case, probe_hit, cap):
    """tests/test_gpu_backward.py _hip_grads with the capacity `cap` in place of the step's own count"""
    opt, xyz, attrs, inp, mlp = case
    dev = torch.device(DEV)
    xyz_d = xyz.to(dev).contiguous()
    pts_t = {k: v.detach().to(dev).reshape(v.shape[1], v.shape[2]).contiguous() for k, v in attrs.items()}
    raydir = inp["raydir"][0].to(dev).contiguous()
    dense = lighting_fast_querier(dev, opt).query_dense(xyz_d[None], xyz.shape[0], float(inp["near"].min()), float(inp["far"].max()), raydir[None],
                                                        inp["campos"].to(dev))
    flat = ops.flatten_mlp(mlp, dev)
    packed = ops.pack_mlp(flat)
    cam = ops.make_camera(inp["campos"][0].numpy(), inp["camrotc2w"][0].numpy(), opt.vsize[2], opt.raydist_mode_unit, bg=inp["bg_color"][0].numpy())
    pts = ops.make_points(xyz_d, pts_t["points_embeding"], pts_t["points_conf"], pts_t["points_dir"], pts_t["points_color"])
    R = raydir.shape[0]
    fwd = ops.render_forward(cam, pts, packed, flat, raydir, dense, R, opt.SR, opt.K, cap, True)
    g = torch.zeros(R, 3, device=dev)
    g[dense["ray_hit"] > 0] = probe_hit.to(dev)
    gflat = torch.zeros_like(flat)
    grads = {k: torch.zeros_like(v) for k, v in pts_t.items()}
    ops.render_backward(cam, pts, packed, flat, raydir, dense, R, opt.SR, opt.K, cap, fwd, g, gflat, grads)
    torch.cuda.synchronize()
    lay, _ = ops.mlp_layout()
    return int(dense["counters"][0].item()), {k: gflat[o:o + int(np.prod(shp))].view(shp).cpu() for k, (o, shp) in lay.items()}


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("name", ["small_k8", "small_k4"])
@pytest.mark.parametrize("n,cap", CALLS)
def test_weight_gradients_at_the_ring_and_grid_edges(n, cap, name, planes):
    case = forced_case(name, n, 120)
    if (name, n) not in _oracle:
        _oracle[(name, n)] = TB._oracle_grads(*case)
    gm_o, _, probe = _oracle[(name, n)]
    old = ops.set_wgrad_planes(planes)
    try:
        count, gm = _grads(case, probe, cap)
    finally:
        ops.set_wgrad_planes(old)
    assert count == n, "the case does not have the forced number of valid samples"
    for k in gm_o:
        TB._check(k, gm[k], gm_o[k])

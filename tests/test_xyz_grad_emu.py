"""xyz_grad (pnerf_point_grads.xyz, k_agg_backward's XYZG instances) on the host emulator (tools/emu): d xyz of the fused backward against
torch.autograd of the float64 yardstick with the point positions as a leaf (oracle/pyref.py render_f64; the query is not differentiated,
as in the reference), in each of the three arithmetics of the input-gradient chain; the other gradients equal those of the run without d xyz;
without the pointer the default instances run."""
import numpy as np
import pytest
import torch

import test_gpu_backward as TB
from emu_util import emu_backend
from gpu_util import hip_render
from pointnerf_amd import config, ops, scenes
from oracle import pyref


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(TB, "DEV", "cpu")
    with emu_backend():
        yield


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    """the saved-activation arena starts as NaN bit patterns: nothing unwritten may reach a result"""
    orig = ops.Arena.take

    def take(self, nbytes, device):
        t = orig(self, nbytes, device)
        t.fill_(0xFF)
        return t
    monkeypatch.setattr(ops.Arena, "take", take)


def _tiny_case(K, SR, size, n=1200, seed=5):
    opt = config.lego_opt(K=K, SR=SR, P=24, max_o=50000, ranges=[-0.3, -0.3, -0.3, 0.3, 0.3, 0.3])
    xyz = torch.from_numpy(scenes.chair_points(n, seed=seed, radius=0.06))
    attrs = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, 32, seed).items()}
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=55.0, x0=400 - size // 2, y0=400 - size // 2, size=size))
    mlp = pyref.init_mlp_params(opt, seed=3, bias_scale=0.1)
    return opt, xyz, attrs, inp, mlp


def _oracle_xyz_grad(opt, xyz, attrs, inp, mlp, probe):
    q = pyref.query(opt, xyz, inp)
    points = dict(xyz=xyz.clone().requires_grad_(True), **{k: v.clone().requires_grad_(True) for k, v in attrs.items()})
    m = {k: v.clone().requires_grad_(True) for k, v in mlp.items()}
    out, pts, _ = pyref.render_f64(opt, points, m, inp, q)
    (out["coarse_raycolor"] * probe.double()[None]).sum().backward()
    return pts["xyz"].grad.float()


def _hip(opt, xyz, attrs, inp, mlp, probe, with_xyz):
    dense, fwd, ctx = hip_render(opt, xyz, attrs, inp, mlp, train=True)
    hit = dense["ray_hit"] > 0
    g = torch.zeros(ctx["R"], 3)
    g[hit] = probe
    gflat = torch.zeros_like(ctx["flat"])
    grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
    if with_xyz:
        grads["xyz"] = torch.zeros(xyz.shape[0], 3)
    ops.render_backward(ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K,
                        ctx["n_valid"], fwd, g, gflat, grads)
    return gflat, grads


@pytest.mark.parametrize("mode", ["mix", "f16", "wg2"])
@pytest.mark.parametrize("K,SR,size", [(8, 12, 5), (3, 10, 4), (12, 8, 4), (1, 6, 5), (16, 6, 3)])
def test_emulated_xyz_grad_matches_float64_autograd(K, SR, size, mode):
    case = _tiny_case(K, SR, size)
    _, _, probe = TB._oracle_grads(*case)
    ref = _oracle_xyz_grad(*case, probe)
    assert float(ref.abs().max()) > 0
    old_ct = old_wg = None
    try:
        if mode == "f16":                       # f16 cross terms (csrc/f16x3.h) in the input-gradient chain
            old_ct = ops.set_cross_terms(16)[0]
        elif mode == "wg2":                     # two-plane weight-gradient mode (f16x3.h arithmetic everywhere)
            old_wg = ops.set_wgrad_planes(2)
        gflat0, g0 = _hip(*case, probe, False)
        gflat1, g1 = _hip(*case, probe, True)
    finally:
        if old_ct is not None:
            ops.set_cross_terms(old_ct)
        if old_wg is not None:
            ops.set_wgrad_planes(old_wg)
    TB._check("points_xyz", g1["xyz"], ref)
    # d xyz leaves the other gradients alone: the same kernels' arithmetic up to the order of the float atomics
    for k in g0:
        s = max(float(g0[k].abs().max()), 1e-8)
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-5 * s, k
    s = max(float(gflat0.abs().max()), 1e-8)
    assert float((gflat1 - gflat0).abs().max()) <= 1e-5 * s


def test_emulated_xyz_pointer_is_null_by_default():
    """pnerf_point_grads.xyz defaults to NULL (every existing caller: the default instances, no d xyz)"""
    from pointnerf_amd import _lib as L
    assert L.PointGrads().xyz is None
    case = _tiny_case(8, 12, 5)
    _, _, probe = TB._oracle_grads(*case)
    gflat, g = _hip(*case, probe, False)
    assert "xyz" not in g and float(g["points_embeding"].abs().max()) > 0

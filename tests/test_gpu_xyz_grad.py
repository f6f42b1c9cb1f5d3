"""xyz_grad on the device: d xyz of the fused backward (k_agg_backward's XYZG instances) against torch.autograd of the float64 yardstick
with the point positions as a leaf, in each of the three arithmetics of the input-gradient chain (bars of tests/test_gpu_backward.py's
point tensors, whose slack covers LeakyReLU-kink flips); and three training steps with trainable positions through the model shell, where
after every step the query on the MOVED cloud must equal the oracle's query of the same positions bit for bit (a stale voxel grid would not)."""
import pytest
import torch

import test_gpu_backward as TB
from cases import build_case
from gpu_util import hip_render
from pointnerf_amd import dist as pdist, ops
from pointnerf_amd.neural_points import NeuralPoints
from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
from pointnerf_amd.optim import FusedAdam
from pointnerf_amd.point_aggregators import PointAggregator
from oracle import pyref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _oracle_xyz_grad(opt, xyz, attrs, inp, mlp, probe):
    q = pyref.query(opt, xyz, inp, nthreads=8)
    points = dict(xyz=xyz.clone().requires_grad_(True), **{k: v.clone().requires_grad_(True) for k, v in attrs.items()})
    m = {k: v.clone().requires_grad_(True) for k, v in mlp.items()}
    out, pts, _ = pyref.render_f64(opt, points, m, inp, q)
    (out["coarse_raycolor"] * probe.double()[None]).sum().backward()
    return pts["xyz"].grad.float()


def _hip(opt, xyz, attrs, inp, mlp, probe, with_xyz):
    dense, fwd, ctx = hip_render(opt, xyz, attrs, inp, mlp, train=True)
    hit = dense["ray_hit"] > 0
    g = torch.zeros(ctx["R"], 3, device=DEV)
    g[hit] = probe.to(DEV)
    gflat = torch.zeros_like(ctx["flat"])
    grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
    if with_xyz:
        grads["xyz"] = torch.zeros(xyz.shape[0], 3, device=DEV)
    ops.render_backward(ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K,
                        ctx["n_valid"], fwd, g, gflat, grads)
    torch.cuda.synchronize()
    return gflat.cpu(), {k: v.cpu() for k, v in grads.items()}


@pytest.mark.parametrize("mode", ["mix", "f16", "wg2"])
@pytest.mark.parametrize("name", ["small_k8", "small_k4"])
def test_xyz_grad_matches_float64_autograd(name, mode):
    case = build_case(name)
    _, _, probe = TB._oracle_grads(*case)
    ref = _oracle_xyz_grad(*case, probe)
    old_ct = old_wg = None
    try:
        if mode == "f16":
            old_ct = ops.set_cross_terms(16)[0]
        elif mode == "wg2":
            old_wg = ops.set_wgrad_planes(2)
        gflat0, g0 = _hip(*case, probe, False)
        gflat1, g1 = _hip(*case, probe, True)
    finally:
        if old_ct is not None:
            ops.set_cross_terms(old_ct)
        if old_wg is not None:
            ops.set_wgrad_planes(old_wg)
    TB._check("points_xyz", g1["xyz"], ref)
    for k in g0:
        s = max(float(g0[k].abs().max()), 1e-8)
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-5 * s, k
    assert float((gflat1 - gflat0).abs().max()) <= 1e-5 * max(float(gflat0.abs().max()), 1e-8)


def test_three_steps_with_trainable_positions_query_the_moved_cloud():
    opt, xyz, attrs, inp, mlp = build_case("small_k8")
    opt.xyz_grad = 1
    agg = PointAggregator(opt).to(DEV)
    agg.load_state_dict(mlp)
    agg.flatten_()
    npnt = NeuralPoints(32, xyz.shape[0], opt, DEV)
    a = {k: v.to(DEV) for k, v in attrs.items()}
    npnt.set_points(xyz.to(DEV), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"],
                    points_conf=a["points_conf"], parameter=True)
    assert npnt.xyz.requires_grad
    model = NeuralPointsRayMarching(aggregator=agg, neural_points=npnt, opt=opt).to(DEV)
    agg.flatten_()
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    pts = [npnt.points_embeding, npnt.points_conf, npnt.points_dir, npnt.points_color, npnt.xyz]
    h_mlp = FusedAdam([p for p in agg.parameters() if p.requires_grad], lr=opt.lr, betas=(0.9, 0.999))
    h_pts = FusedAdam(pts, lr=opt.plr, betas=(0.9, 0.999))
    # the oracle: the same steps with torch.optim.Adam, xyz a leaf of the float32 oracle render
    om = {k: v.clone().requires_grad_(True) for k, v in mlp.items()}
    oa = {k: v.clone().requires_grad_(True) for k, v in attrs.items()}
    ox = xyz.clone().requires_grad_(True)
    o_mlp = torch.optim.Adam(list(om.values()), lr=opt.lr, betas=(0.9, 0.999))
    o_pts = torch.optim.Adam(list(oa.values()) + [ox], lr=opt.plr, betas=(0.9, 0.999))
    x0 = xyz.clone()
    for step in range(3):
        h_mlp.zero_grad(set_to_none=True); h_pts.zero_grad(set_to_none=True)
        out = model(**d)
        # the query of THIS step ran on the current cloud: its indices equal the oracle's query of the same positions, bit for bit
        cur = npnt.xyz.detach().reshape(-1, 3).cpu()
        q = pyref.query(opt, cur, inp, nthreads=8)
        hit = model.neural_points.querier.last_dense["ray_hit"].cpu() > 0
        pidx = model.neural_points.querier.last_dense["sample_pidx"].cpu()[hit]
        assert torch.equal(pidx[None], q["sample_pidx"]), "step %d queried a stale grid" % step
        loss = pdist.hot_path_loss(opt, out, d["gt_image"])
        loss.backward()
        assert npnt.xyz.grad is not None and float(npnt.xyz.grad.abs().max()) > 0
        h_mlp.step(); h_pts.step()
        o_mlp.zero_grad(); o_pts.zero_grad()
        ro = pyref.render(opt, dict(xyz=ox, **oa), om, inp, nthreads=8)
        pyref.training_loss(opt, ro, inp).backward()
        o_mlp.step(); o_pts.step()
        print("step", step, "loss", float(loss.detach()))
    moved = npnt.xyz.detach().reshape(-1, 3).cpu()
    assert float((moved - x0).abs().max()) > 0.5 * opt.plr
    # xyz and the embedding follow torch.optim.Adam around the oracle (Adam moves an element by ~plr per step; kink flips by up to 2 plr)
    for got, ref in ((moved, ox.detach()), (npnt.points_embeding.detach().cpu(), oa["points_embeding"].detach())):
        e = (got - ref).abs()
        frac = float((e > 0.05 * opt.plr).float().mean())
        print("max err %.2e  frac > 5%% of plr %.1e" % (float(e.max()), frac))
        assert float(e.max()) <= 2.0 * opt.plr * 3 and frac <= 2e-3


def test_prune_keeps_positions_trainable():
    opt, xyz, attrs, inp, mlp = build_case("small_k8")
    opt.xyz_grad = 1
    npnt = NeuralPoints(32, xyz.shape[0], opt, DEV)
    a = {k: v.to(DEV) for k, v in attrs.items()}
    npnt.set_points(xyz.to(DEV), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"],
                    points_conf=a["points_conf"], parameter=True)
    npnt.prune(float(a["points_conf"].median()))
    assert npnt.xyz.requires_grad and getattr(npnt.xyz, "pnerf_point_xyz", False)

"""Per-point Rw2c frames (scene editing): the seeded frame generator, the torch-CPU restatement of the reference's per-point branch
(models/aggregators/point_aggregators.py:492-496,506,526,566; frames gathered at models/neural_points/neural_points.py:717) and the
checks that tests/test_editing_emu.py (host emulator) and tests/test_gpu_editing.py (device) share.

Semantics restated (F[p] = the [3,3] frame of point p, empty slots read point 0):
  row of neighbor slot k, p = max(pidx[s,k], 0):  dists[:3] -> F[p] dw,  stored direction -> q = F[p] dir[p],  the perspective
      components and the raw weight 1/|dw| untouched;
  sample s:  view direction v = F[max(pidx[s,0], 0)] raydir  -- the frame of SLOT 0 -- into PE4(view) of the colour branch AND into every
      row's extras (q - v, q.v): a row mixes its own frame with slot 0's (the reference's quirk, kept).
tests/golden/editing_frames.npz pins the restatement against the reference's own PointAggregator (tests/golden/make_editing_golden.py)."""
import os

import torch
import torch.nn.functional as F

from cases import build_case
from oracle import pyref

CASES = ("small_k4", "small_k8")        # 900 points / 100 rays / SR 16 / K 4 and 1 500 / 144 / 24 / 8: partial 64-row tiles, every row class
PARTS = 3
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "editing_frames.npz")
BAR = 1e-4                              # the project's forward bar


def rotations(parts=PARTS, seed=0):
    """[parts,3,3] proper rotations, the first one the identity"""
    g = torch.Generator().manual_seed(1000 + seed)
    rots = [torch.eye(3)]
    for _ in range(parts - 1):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        if torch.det(q) < 0:
            q[:, 0] = -q[:, 0]
        rots.append(q.contiguous())
    return torch.stack(rots)


def make_frames(n_points, parts=PARTS, seed=0):
    """(frames [N,3,3], part of every point [N]): the parts are assigned to the points at random, so most samples mix parts"""
    g = torch.Generator().manual_seed(2000 + seed)
    part = torch.randint(0, parts, (n_points,), generator=g)
    return rotations(parts, seed)[part].contiguous(), part


def case_frames(name):
    n = build_case(name)[1].shape[0]
    return make_frames(n, seed=CASES.index(name))[0]


def gather_frames(frames, pidx):
    """neural_points.py:708-717: [N,3,3] -> [1,R,SR,K,3,3], empty slots read point 0"""
    return frames[pidx.clamp(min=0).long().view(-1)].view(tuple(pidx.shape) + (3, 3))


def aggregate_frames(opt, mlp, nb, loc_p, loc_w, ray_dirs, Fg):
    """pyref.aggregate with one frame per gathered neighbor, Fg [1,R,SR,K,3,3].  Returns (output [1,R,SR,4], ray_valid, weight,
    conf_coefficient) like pyref.aggregate."""
    mask = nb["mask"]
    B, R, SR, K = mask.shape
    dt = loc_w.dtype
    Fg = Fg.to(dt)
    ray_valid = mask.any(dim=-1)
    out = torch.zeros(B, R, SR, 4, dtype=dt)
    xp, lp = nb["xyz_pers"], loc_p[..., None, :]
    dists = torch.cat([nb["xyz"] - loc_w[..., None, :],
                       torch.stack([xp[..., 0] * xp[..., 2] - lp[..., 0] * lp[..., 2],
                                    xp[..., 1] * xp[..., 2] - lp[..., 1] * lp[..., 2],
                                    xp[..., 2] - lp[..., 2]], dim=-1)], dim=-1)
    w = mask.to(dt) / torch.clamp(torch.linalg.norm(dists[..., :3], dim=-1), min=1e-6)
    w = w / torch.clamp(w.sum(dim=-1, keepdim=True), min=1e-8)
    conf = nb["conf"][..., 0]
    conf_c = conf - (conf - conf.clamp(1e-4, 1.0)).detach()
    if ray_valid.sum() == 0:
        return out, ray_valid, w, conf_c
    wc = w * conf_c
    mf, vf = mask.view(-1), ray_valid.view(-1)
    Ft_row = Fg.transpose(-1, -2).reshape(-1, 3, 3)[mf]                       # :492,496  the row's own frame, transposed
    Ft_ray = Fg.transpose(-1, -2)[:, :, :, 0].reshape(-1, 3, 3)               # :495      slot 0's frame of every sample
    d = dists.view(-1, 6)[mf]
    d = torch.cat([(d[:, None, :3] @ Ft_row).squeeze(-2), d[:, 3:]], dim=-1)  # :526
    d = pyref.positional_encoding(d, opt.dist_xyz_freq)
    feat = nb["emb"].reshape(-1, nb["emb"].shape[-1])[mf]
    feat = torch.cat([feat, pyref.positional_encoding(feat, opt.num_feat_freqs), d], dim=-1)
    act = lambda x: F.leaky_relu(x, 0.01)
    lin = lambda x, k: F.linear(x, mlp[k + ".weight"], mlp[k + ".bias"])
    feat = act(lin(act(lin(feat, "block1.0")), "block1.2"))
    view = (ray_dirs.reshape(-1, 1, 3) @ Ft_ray).squeeze(-2)                  # :506
    view_pe = pyref.positional_encoding(view, opt.num_viewdir_freqs, ori=True)[:, 3:]
    view_k = view[:, None, :].expand(-1, K, -1).reshape(-1, 3)[mf]            # :567-569
    pdir = (nb["dir"].reshape(-1, 1, 3)[mf] @ Ft_row).squeeze(-2)             # :566
    feat = torch.cat([feat, nb["color"].reshape(-1, 3)[mf], pdir - view_k, (pdir * view_k).sum(-1, keepdim=True)], dim=-1)
    feat = act(lin(act(lin(feat, "block3.0")), "block3.2"))
    alpha = F.softplus(lin(feat, "alpha_branch.0") - 1)
    n_all = B * R * SR * K
    rows = mf.nonzero()[:, 0]
    a_full = torch.zeros(n_all, 1, dtype=dt).index_put((rows,), alpha)
    f_full = torch.zeros(n_all, feat.shape[-1], dtype=dt).index_put((rows,), feat)
    wk = wc.reshape(-1, K, 1)
    sigma = (a_full.view(-1, K, 1) * wk).sum(dim=1)[vf]
    fs = (f_full.view(-1, K, feat.shape[-1]) * wk).sum(dim=1)[vf]
    c = torch.cat([fs, view_pe[vf]], dim=-1)
    c = act(lin(c, "color_branch.0")); c = act(lin(c, "color_branch.2")); c = act(lin(c, "color_branch.4"))
    rgb = torch.sigmoid(lin(c, "color_branch.6")) * (1 + 2 * 0.001) - 0.001
    out = out.view(-1, 4).index_put((vf.nonzero()[:, 0],), torch.cat([sigma, rgb], dim=-1)).view(B, R, SR, 4)
    return out, ray_valid, w, conf_c


def render_frames(opt, points, mlp, inp, frames, q=None):
    """pyref.render with per-point frames [N,3,3]: the oracle route of the editing tests"""
    with torch.no_grad():
        if q is None:
            q = pyref.query(opt, points["xyz"], inp)
        nb = pyref.gather_neighbors(points, q["sample_pidx"], inp["camrotc2w"][0], inp["campos"][0])
        feats, ray_valid, w, conf_c = aggregate_frames(opt, mlp, nb, q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"],
                                                       gather_frames(frames, q["sample_pidx"]))
        rd = pyref.ray_dist(opt, q["sample_loc"], ray_valid)
        color, _, opacity, acc, bw, bg_t = pyref.ray_march(rd, ray_valid, feats, inp["bg_color"])
    return dict(coarse_raycolor=color, coarse_point_opacity=opacity, coarse_is_background=bg_t, ray_mask=q["ray_mask"], weight=w,
                blend_weight=bw, conf_coefficient=conf_c, decoded_features=feats, ray_valid=ray_valid, query=q, neighbors=nb)


_REF = {}


def reference(name):
    """(case, frames, restatement result) of a case, computed once and shared; callers leave it unchanged"""
    if name not in _REF:
        case = build_case(name)
        opt, xyz, attrs, inp, mlp = case
        frames = case_frames(name)
        _REF[name] = (case, frames, render_frames(opt, dict(xyz=xyz, **attrs), mlp, inp, frames))
    return _REF[name]


# ------------------------------------------------------------------------------------------------- shared by the emulator and device tests
def build_model(name, dev, frames=None, editing=True):
    """(model, d) -- the fused NeuralPointsRayMarching of a case on ``dev``; ``frames`` [N,3,3] go in through the public entry of a composed
    scene (``editing_set_points``) or, with editing=False, through ``set_points(Rw2c=...)``"""
    from pointnerf_amd.neural_points import NeuralPoints
    from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
    from pointnerf_amd.point_aggregators import PointAggregator
    opt, xyz, attrs, inp, mlp = reference(name)[0]
    dev = torch.device(dev)
    agg = PointAggregator(opt).to(dev)
    agg.load_state_dict(mlp)
    agg.flatten_()
    npnt = NeuralPoints(32, xyz.shape[0], opt, dev)
    a = {k: v.to(dev) for k, v in attrs.items()}
    kw = dict(points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"],
              Rw2c=None if frames is None else frames.to(dev))
    if editing:
        npnt.editing_set_points(xyz.to(dev), a["points_embeding"], **kw)
    else:
        npnt.set_points(xyz.to(dev), a["points_embeding"], parameter=True, **kw)
    model = NeuralPointsRayMarching(aggregator=agg, neural_points=npnt, opt=opt)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return model, d


def fused_outputs(model, d):
    """decoded / weight [R,SR,*] dense over the submitted rays, and the model's compacted outputs"""
    with torch.no_grad():
        out = model(**d)
        dense = model.render_dense(d["campos"], d["raydir"], d["camrotc2w"], d["near"], d["far"], d["bg_color"])
    return out, dict(ray_color=dense[0], opacity=dense[1], decoded=dense[4], weight=dense[5], dense=dense[7])


def errors(out, dn, ref):
    """max abs differences of the fused path to the restatement: decoded / weight over the hit rays' samples, opacity, ray colour"""
    hit = (dn["dense"]["ray_hit"] > 0).cpu()
    e = dict(decoded=float((dn["decoded"].cpu()[hit][None] - ref["decoded_features"]).abs().max()),
             weight=float((dn["weight"].cpu()[hit][None] - ref["weight"]).abs().max()),
             opacity=float((out["coarse_point_opacity"].cpu() - ref["coarse_point_opacity"]).abs().max()),
             raycolor=float((out["coarse_raycolor"].cpu() - ref["coarse_raycolor"]).abs().max()))
    return e


def check_fused(name, dev):
    case, frames, ref = reference(name)
    model, d = build_model(name, dev, frames)
    out, dn = fused_outputs(model, d)
    assert torch.equal(out["ray_mask"].cpu(), ref["ray_mask"])
    e = errors(out, dn, ref)
    print(name, "fused vs restatement:", e)
    assert all(v <= BAR for v in e.values()), e
    return e


def check_level1(name, dev):
    """NeuralPoints.forward (gathers the frames) -> PointAggregator.forward -> ray march, module by module"""
    import test_gpu_level1 as T1
    case, frames, ref = reference(name)
    model, d = build_model(name, dev, frames)
    with torch.no_grad():
        out = T1._level1_forward(case[0], model.aggregator, model.neural_points, d)
    assert torch.equal(out["ray_mask"].cpu(), ref["ray_mask"])
    e = {k: float((out[k].cpu() - ref[rk]).abs().max()) for k, rk in (("decoded_features", "decoded_features"), ("coarse_raycolor", "coarse_raycolor"),
                                                                        ("coarse_point_opacity", "coarse_point_opacity"))}
    e["weight"] = float((out["weight"].cpu() - ref["weight"]).abs().max()) if out["weight"] is not None else 0.0
    print(name, "level-1 vs restatement:", e)
    assert all(v <= BAR for v in e.values()), e


def check_training_raises(name, dev):
    import pytest
    import test_gpu_level1 as T1
    case, frames, ref = reference(name)
    model, d = build_model(name, dev, frames, editing=False)
    assert model.neural_points.points_embeding.requires_grad
    with pytest.raises(NotImplementedError, match="Rw2c"):
        model(**d)                                                   # gradients enabled: a training forward
    with pytest.raises(NotImplementedError, match="Rw2c"):
        T1._level1_forward(case[0], model.aggregator, model.neural_points, d)

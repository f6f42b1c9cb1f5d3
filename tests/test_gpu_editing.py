"""Per-point Rw2c frames (scene editing) on the device: the FRAMES instances of k_agg_forward / k_color_forward against the torch restatement
of the reference's per-point branch (tests/editing_case.py; pinned to the reference's own PointAggregator by tests/golden/editing_frames.npz).
Shapes: small_k4 (900 points, 100 rays, SR 16, K 4) and small_k8 (1 500 points, 144 rays, SR 24, K 8) -- partial 64-row tiles and all three
row classes.  Bars: the project's forward bar 1e-4 on sigma / RGB per sample, weights, opacity and ray colour; exact equality
where the arithmetic is exact (identity frames, frames nobody reads, repeated launches)."""
import numpy as np
import pytest
import torch

import editing_case as E
from gpu_util import DEV
from oracle import pyref

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", E.CASES)
def test_fused_forward_with_frames_matches_the_restatement(name):
    E.check_fused(name, DEV)


@pytest.mark.parametrize("name", E.CASES)
def test_level1_chain_with_frames_matches_the_restatement(name):
    E.check_level1(name, DEV)


def _dense(name, frames, editing=True):
    model, d = E.build_model(name, DEV, frames, editing=editing)
    out, dn = E.fused_outputs(model, d)
    return out, dn


@pytest.mark.parametrize("name", E.CASES)
def test_identity_frames_equal_the_uniform_path_bit_for_bit(name):
    """a rotation by exact 0 / 1 entries is exact in any order of the sums: a difference is an indexing bug"""
    n = E.reference(name)[0][1].shape[0]
    out_u, dn_u = _dense(name, None)
    out_f, dn_f = _dense(name, torch.eye(3)[None].repeat(n, 1, 1))
    for k in ("decoded", "weight", "opacity", "ray_color"):
        assert torch.equal(dn_u[k], dn_f[k]), k
    assert torch.equal(out_u["coarse_raycolor"], out_f["coarse_raycolor"]) and torch.equal(out_u["ray_mask"], out_f["ray_mask"])
    assert float(dn_u["decoded"].abs().max()) > 0


@pytest.mark.parametrize("name", E.CASES)
def test_frame_of_point_0_does_not_reach_samples_through_empty_slots(name):
    """empty slots read point 0 (and its frame) with weight 0: a distinctive frame on point 0 leaves every sample unchanged that does not
    have point 0 as a real neighbor; the others still follow the restatement"""
    (opt, xyz, attrs, inp, mlp), frames, ref = E.reference(name)
    other = frames.clone()
    other[0] = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) @ E.rotations()[2]
    assert not torch.equal(other[0], frames[0])
    out_a, dn_a = _dense(name, frames)
    out_b, dn_b = _dense(name, other)
    pidx = dn_a["dense"]["sample_pidx"]
    valid = (pidx >= 0).any(-1)
    uses0 = (pidx == 0).any(-1)
    clean = valid & ~uses0
    assert int((clean & (pidx < 0).any(-1)).sum()) > 0                     # empty slots exist in samples that point 0 is no neighbor of
    assert torch.equal(dn_a["decoded"][clean], dn_b["decoded"][clean]) and torch.equal(dn_a["weight"], dn_b["weight"])
    ref_b = E.render_frames(opt, dict(xyz=xyz, **attrs), mlp, inp, other, q=ref["query"])
    e = E.errors(out_b, dn_b, ref_b)
    assert all(v <= E.BAR for v in e.values()), e


def test_two_launches_give_the_same_bits():
    _, frames, _ = E.reference("small_k8")
    model, d = E.build_model("small_k8", DEV, frames)
    a = E.fused_outputs(model, d)[1]
    b = E.fused_outputs(model, d)[1]
    for k in ("decoded", "weight", "opacity", "ray_color"):
        assert torch.equal(a[k], b[k]), k


def test_training_with_frames_raises():
    E.check_training_raises("small_k4", DEV)


def test_settings_without_a_frames_instance_are_refused_by_name():
    from pointnerf_amd import ops
    _, frames, _ = E.reference("small_k4")
    model, d = E.build_model("small_k4", DEV, frames)
    old = ops.set_inference_products(2)
    try:
        with pytest.raises(NotImplementedError, match="set_inference_products"), torch.no_grad():
            model(**d)
    finally:
        ops.set_inference_products(old)
    oldc = ops.set_cross_terms(8, where=5)
    try:
        with pytest.raises(NotImplementedError, match="cross"), torch.no_grad():
            model(**d)
    finally:
        ops.set_cross_terms(oldc[0], where=oldc[1])
    with torch.no_grad():
        model(**d)


def test_render_image_with_frames_matches_the_oracle_route():
    """eval_loop.render_image (chunked) on a composed scene == the restatement rendered ray by ray (tests/test_gpu_level1.py's eval test
    with frames)"""
    from pointnerf_amd import eval_loop
    (opt, xyz, attrs, inp, mlp), frames, _ = E.reference("small_k8")
    model, d = E.build_model("small_k8", DEV, frames)
    intr = inp["intrinsic"][0].clone()
    intr[0, 2] -= 388.0; intr[1, 2] -= 390.0
    h, w = 20, 24
    img, hit = eval_loop.render_image(model, d["campos"], d["camrotc2w"], intr, h, w, d["near"], d["far"], d["bg_color"], chunk=157)
    sub = dict(inp)
    sub["raydir"] = eval_loop.rays_from_pixels(eval_loop.pixel_grid(h, w, torch.device("cpu")), intr, inp["camrotc2w"])
    ref = E.render_frames(opt, dict(xyz=xyz, **attrs), mlp, sub, frames)
    full = pyref.fill_invalid(ref, sub)
    assert torch.equal(hit.cpu(), ref["ray_mask"][0] > 0) and int(hit.sum()) > 50
    assert float((img.cpu().reshape(-1, 3) - full["coarse_raycolor"][0]).abs().max()) <= E.BAR


def test_probe_hole_fused_with_frames_matches_the_oracle_route(tmp_path):
    """probe.probe_hole(fused=True) through the model shell on a composed scene (model.set_points(..., editing=True)) against the
    restatement's probe outputs pushed through the index-loop statement of the candidate rule (tests/test_gpu_model_shell.py's probe test
    with frames)"""
    import test_gpu_model_shell as TS
    from pointnerf_amd import probe, scenes
    H = W = 800
    opt, m, xyz, attrs, mlp, _, seed = TS._scene("small_k8", tmp_path, is_train=0, prob_mul=0.4, prob_num_step=1)
    frames = E.case_frames("small_k8")
    a = {k: v.to(DEV) for k, v in attrs.items()}
    m.set_points(xyz.to(DEV), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"],
                 Rw2c=frames.to(DEV), editing=True)
    assert m.neural_points.Rw2c.shape == (xyz.shape[0], 3, 3)
    size = 44
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=400 - size // 2, y0=400 - size // 2, size=size))
    points = dict(xyz=xyz, **attrs)
    ref = E.render_frames(opt, points, mlp, inp, frames, q=pyref.query(opt, xyz, inp, nthreads=8))
    with torch.no_grad():
        pr = pyref.probe_outputs(ref, points)
    hit = ref["ray_mask"][0] > 0
    assert 50 < int(hit.sum()) < hit.numel() - 50
    pix = inp["pixel_idx"][0].long()

    def to_map(compact, c):
        t = np.zeros((H, W, c), np.float32)
        t[pix[hit, 1].numpy(), pix[hit, 0].numpy()] = compact[0].numpy()
        return t
    maps = {k: to_map(v, v.shape[-1]) for k, v in pr.items()}
    col = np.zeros((H, W, 3), np.float32); col[pix[:, 1].numpy(), pix[:, 0].numpy()] = pyref.fill_invalid(ref, inp)["coarse_raycolor"][0].numpy()
    rm = np.zeros((H, W), np.float32); rm[pix[:, 1].numpy(), pix[:, 0].numpy()] = hit.float().numpy()
    edge = np.zeros((H, W), bool); edge[pix[:, 1].numpy(), pix[:, 0].numpy()] = True
    gt = np.zeros((H, W, 3), np.float32); gt[pix[:, 1].numpy(), pix[:, 0].numpy()] = inp["gt_image"][0].numpy()
    op = np.sort(maps["ray_max_shading_opacity"][..., 0][rm > 0])           # a threshold in the widest gap of the opacities: rounding flips no candidate
    gaps = np.diff(op)
    lo = len(op) // 4
    j = lo + int(np.argmax(gaps[lo:3 * len(op) // 4]))
    thresh = float(0.5 * (op[j] + op[j + 1]))
    assert gaps[j] > 1e-3 * thresh
    mask = pyref.probe_hole_mask(rm, maps["ray_max_shading_opacity"][..., 0], maps["ray_max_far_dist"][..., 0], col, gt,
                                 inp["bg_color"].numpy().reshape(1, 3), edge, thresh)
    assert 5 < mask.sum() < (rm > 0).sum()
    got = probe.probe_hole(m, [dict(inp, id=0)], opt, H, W, test_steps=0, opacity_thresh=thresh, frame_ids=[0], chunk=700, fused=True)
    xyz_a, emb_a, col_a, dir_a, conf_a = [t.cpu().numpy() for t in got]
    assert xyz_a.shape == (int(mask.sum()), 3) and emb_a.shape == (int(mask.sum()), 32)
    for arr, k, s in ((xyz_a, "ray_max_sample_loc_w", 1.0), (emb_a, "shading_avg_embedding", 1.0), (col_a, "shading_avg_color", 1.0),
                      (dir_a, "shading_avg_dir", 1.0), (conf_a, "shading_avg_conf", 0.4)):
        assert float(np.abs(arr - maps[k][mask] * np.float32(s)).max()) <= E.BAR, k

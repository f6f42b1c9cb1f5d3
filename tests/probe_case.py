"""Shared inputs of the probe-pass tests (tests/test_probe_emu.py on the host emulator, tests/test_gpu_probe_fused.py on the device):
seeded SYNTHETIC inputs of pnerf_probe_rays / pnerf_probe_hole_mask, a torch restatement of the reference's statements
(models/neural_points_volumetric_model.py:331-352) that spells out "first index among the maxima", and the bars.

Ray cases (R, SR, K): one sample; one partial 64-chunk; the chunk boundary from below (63), on it (64) and above (65); three chunks (130).
R is never a multiple of the four rays of a workgroup except 1 < 4 itself: the last workgroup is partial.  Ray r of a case is, by r % 4,
  0  random opacities;
  1  an exact tie of the maximum: at sample 40 (lane 40) and at the LAST sample of the row (in another 64-chunk where SR > 64, in a lower
     lane than 40 at SR = 65 / 130): the lower index must win whatever the reduction tree does;
  2  all opacities 0 (sample 0 is the first maximum);
  3  a ray that MISSED (ray_hit 0) whose opacity / weight / location rows are NaN: its outputs must be 0.
and, by r % 3, its neighbor table has no empty slot / some (-1) / only empty slots.  The cloud has 50 points with confidences in
[-0.5, 1.5] (both sides of gradient_clamp's [1e-4, 1]); point 0 -- what an empty slot reads -- sits in the middle of the sample locations
(``near0``: nearer than the real neighbors of some rays) or far outside (farther than all of them).

Bars (derived, not tuned):
  ray_max_shading_opacity, ray_max_sample_loc_w   bit-equal (selections);
  ray_max_far_dist    4 * 2^-24 relative: three squares, two additions and a square root in fp32 against torch.norm's fp32, with or without
                      FMA contraction, is ~1.25 ulp on either side;
  shading_avg_*       2e-6 * sum_k |w_k row_k| + 1e-30 per element: K + 1 <= 17 fp32 roundings of 2^-24 give 1.0e-6 against the exact sum
                      (formed here in float64 from the fp32 w_k); the factor 2 leaves room for a second fp32 evaluation on the other side
                      (fused against unfused on the device)."""
import numpy as np
import torch

RAY_CASES = [(1, 1, 1), (5, 24, 8), (7, 63, 4), (7, 64, 12), (9, 65, 16), (6, 130, 8)]
N_POINTS = 50
KEYS = ("ray_max_shading_opacity", "ray_max_sample_loc_w", "ray_max_far_dist", "shading_avg_color", "shading_avg_dir", "shading_avg_conf",
        "shading_avg_embedding")
AVG_KEYS = ("shading_avg_color", "shading_avg_dir", "shading_avg_conf", "shading_avg_embedding")
EPS = 2.0 ** -24


def points(near0, seed=7):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(N_POINTS, 3, generator=g) * 2 - 1
    xyz[0] = torch.tensor([0.02, -0.01, 0.03]) if near0 else torch.tensor([5.0, 5.0, 5.0])
    return dict(xyz=xyz, points_embeding=torch.randn(N_POINTS, 32, generator=g), points_conf=torch.rand(N_POINTS, 1, generator=g) * 2 - 0.5,
                points_dir=torch.rand(N_POINTS, 3, generator=g) * 2 - 1, points_color=torch.rand(N_POINTS, 3, generator=g))


def ray_case(R, SR, K, seed=0):
    """dict(opacity [R,SR], weight [R,SR,K], sample_loc [R,SR,3], sample_pidx [R,SR,K] i32, ray_hit [R] i32) on the CPU"""
    g = torch.Generator().manual_seed(1000 * R + 10 * SR + K + seed)
    op = torch.rand(R, SR, generator=g) * 0.9
    w = torch.rand(R, SR, K, generator=g)
    loc = torch.rand(R, SR, 3, generator=g) - 0.5
    pidx = torch.randint(0, N_POINTS, (R, SR, K), generator=g, dtype=torch.int32)
    hit = torch.ones(R, dtype=torch.int32)
    for r in range(R):
        if r % 3 == 1:
            pidx[r][torch.rand(SR, K, generator=g) < 0.4] = -1
        elif r % 3 == 2:
            pidx[r] = -1
        if r % 4 == 1:
            op[r, min(40, SR - 1)] = 0.97
            op[r, SR - 1] = 0.97
        elif r % 4 == 2:
            op[r] = 0.0
        elif r % 4 == 3:
            hit[r] = 0
            op[r], w[r], loc[r] = float("nan"), float("nan"), float("nan")
    return dict(opacity=op, weight=w, sample_loc=loc, sample_pidx=pidx, ray_hit=hit)


def restate(pts, c):
    """(outputs {key: [R, C] f32}, scales {avg key: [R, C] f64 = sum_k |w_k row_k|}) of neural_points_volumetric_model.py:331-352 on the dense
    tensors; rays with ray_hit <= 0 are zero rows (:121-122).  The averages are summed in float64 from the fp32 factors."""
    op, hit = c["opacity"], c["ray_hit"] > 0
    R, SR = op.shape
    rows = torch.arange(R)
    mx = torch.max(torch.nan_to_num(op, nan=-1.0), dim=-1).values
    ind = torch.where(op == mx[:, None], torch.arange(SR)[None].expand(R, SR), torch.full((R, SR), SR)).min(-1).values      # FIRST index among the maxima
    ind = torch.where(hit, ind, torch.zeros_like(ind))
    loc = c["sample_loc"][rows, ind]                                              # [R,3]
    p = c["sample_pidx"][rows, ind].clamp(min=0).long()                           # [R,K]   empty slots read point 0
    w = c["weight"][rows, ind] * pts["points_conf"][:, 0][p].clamp(min=1e-4, max=1.0)       # fp32 product, as the reference forms it
    out = {"ray_max_shading_opacity": op[rows, ind][:, None], "ray_max_sample_loc_w": loc,
           "ray_max_far_dist": torch.norm(pts["xyz"][p] - loc[:, None, :], dim=-1).min(-1).values[:, None]}
    scale = {}
    for k, name in zip(AVG_KEYS, ("points_color", "points_dir", "points_conf", "points_embeding")):
        terms = w.double()[..., None] * pts[name][p].double()                    # [R,K,C] exact products
        out[k] = terms.sum(1).float()
        scale[k] = torch.where(hit[:, None], terms.abs().sum(1), torch.zeros((), dtype=torch.float64))
    for k in out:
        out[k] = torch.where(hit[:, None], out[k], torch.zeros(()))
    return out, scale


def check(got, ref, scale, tag=""):
    """the bars of the module docstring; got / ref {key: [R, C]} on the CPU"""
    for k in ("ray_max_shading_opacity", "ray_max_sample_loc_w"):
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (tag, k, got[k], ref[k])
    a, b = got["ray_max_far_dist"].double(), ref["ray_max_far_dist"].double()
    assert a.shape == b.shape and bool(((a - b).abs() <= 4 * EPS * b.abs()).all()), (tag, "ray_max_far_dist", float(((a - b).abs() / b.abs().clamp(min=1e-30)).max()))
    for k in AVG_KEYS:
        a, b = got[k].double(), ref[k].double()
        assert a.shape == b.shape, (tag, k, a.shape, b.shape)
        bar = 2e-6 * scale[k] + 1e-30
        assert bool(((a - b).abs() <= bar).all()), (tag, k, float(((a - b).abs() / bar).max()))


def assert_case_covers(pts, c, near0):
    """the generator's own promises, so that a change of seeds cannot quietly drop a case"""
    R, SR = c["opacity"].shape
    ref, _ = restate(pts, c)
    if R >= 4:
        assert int(c["ray_hit"][3]) == 0 and bool(torch.isnan(c["opacity"][3]).all())
        first = min(40, SR - 1)
        assert float(c["opacity"][1, first]) == float(c["opacity"][1, SR - 1]) == float(c["opacity"][1].max())
        assert torch.equal(ref["ray_max_sample_loc_w"][1], c["sample_loc"][1, first]) and torch.equal(ref["ray_max_sample_loc_w"][2], c["sample_loc"][2, 0])
        empty = (c["sample_pidx"] < 0)
        assert not bool(empty[0].any()) and bool(empty[1].any()) and not bool(empty[1].all()) and bool(empty[2].all())
        # ray 2 reads only point 0: its distance is point 0's; ray 1 / 4 have real neighbors next to empty slots
        d0 = torch.norm(pts["xyz"][0] - ref["ray_max_sample_loc_w"], dim=-1)
        assert abs(float(ref["ray_max_far_dist"][2, 0]) - float(d0[2])) <= 1e-6
        if near0:
            assert float(d0[2]) < 1.0
        else:
            assert float(d0.min()) > 5.0 and float(ref["ray_max_far_dist"][0, 0]) < 3.0
    conf = pts["points_conf"]
    assert bool((conf < 1e-4).any()) and bool((conf > 1.0).any())


# ---------------------------------------------------------------------------------------------------- the candidate mask
MASK_CASES = [(1, 1), (5, 7), (16, 16)]
OPACITY_THRESH, FAR_THRESH = 0.4, 0.5


def mask_case(H, W, seed=0):
    """maps of one view for pnerf_probe_hole_mask: dict(ray_mask [H,W,1] i8, ray_max_shading_opacity / ray_max_far_dist [H,W,1], coarse_raycolor
    [H,W,3], gt [H,W,3], edge [H,W] bool, bg [1,3]).  Misses sit in the corners, on the edges and inside; `edge` leaves out the last column and a
    few inner pixels; |gt - bg| is 0, 0.0015 or 0.004 and |gt - colour| 0.05 or 0.2 -- none within 1e-4 relative of the rule's 0.002 / 0.1
    (asserted below, on the fp32 norms the kernel forms)."""
    g = torch.Generator().manual_seed(100 * H + W + seed)
    hit = torch.rand(H, W, generator=g) < 0.65
    if H * W == 1:
        hit[0, 0] = True
    else:
        hit[0, 0], hit[0, W - 1], hit[H - 1, 0] = False, False, True
        hit[H // 2, 0], hit[0, W // 2], hit[H - 1, W - 1] = False, False, False
        hit[H // 2, W // 2], hit[H // 2, W // 2 - 1] = False, True
    edge = torch.ones(H, W, dtype=torch.bool)
    if W > 1:
        edge[:, W - 1] = False
        edge[torch.rand(H, W, generator=g) < 0.1] = False
        edge[H // 2, W // 2] = True
    bg = torch.tensor([[1.0, 1.0, 1.0]])
    unit = lambda t: t / torch.norm(t, dim=-1, keepdim=True)
    d = unit(torch.rand(H, W, 3, generator=g) + 0.1)
    mag = torch.tensor([0.0, 0.0015, 0.004])[torch.randint(0, 3, (H, W), generator=g)]
    mag[H // 2, W // 2] = 0.004
    gt = (bg - d * mag[..., None]) * edge[..., None]                  # (zero outside the pixels the view has rays for, like probe_hole's)
    d2 = unit(torch.rand(H, W, 3, generator=g) - 0.5)
    mag2 = torch.tensor([0.05, 0.2])[torch.randint(0, 2, (H, W), generator=g)]
    col = gt + d2 * mag2[..., None]
    c = dict(ray_mask=hit.to(torch.int8)[..., None].contiguous(), ray_max_shading_opacity=torch.rand(H, W, 1, generator=g),
             ray_max_far_dist=torch.rand(H, W, 1, generator=g), coarse_raycolor=col.contiguous(), gt=gt.contiguous(), edge=edge, bg=bg)
    n1 = torch.sqrt(((gt - bg) ** 2).sum(-1))
    n2 = torch.sqrt(((gt - col) ** 2).sum(-1))
    assert bool(((n1 - 0.002).abs() > 1e-4 * 0.002).all()) and bool(((n2 - 0.1).abs() > 1e-4 * 0.1).all())
    assert bool(((c["ray_max_far_dist"] - FAR_THRESH).abs() > 1e-6).all()) and bool(((c["ray_max_shading_opacity"] - OPACITY_THRESH).abs() > 1e-6).all())
    if H * W > 1:
        assert bool((n1[edge & ~hit] > 0.002).any()) and bool((n1[edge & ~hit] < 0.002).any()) and bool((~edge & ~hit).any())
    return c


def mask_references(c, far_thresh):
    """(probe.hole_mask on the case's own tensors, pyref.probe_hole_mask on numpy copies): two [H,W] bool arrays"""
    from oracle import pyref
    from pointnerf_amd import probe
    a = probe.hole_mask({k: c[k] for k in ("ray_mask", "ray_max_shading_opacity", "ray_max_far_dist", "coarse_raycolor")}, c["gt"], c["bg"].to(c["gt"].device),
                        c["edge"], OPACITY_THRESH, far_thresh)
    n = lambda t: t.detach().cpu().numpy()
    b = pyref.probe_hole_mask(n(c["ray_mask"])[..., 0].astype(np.float32), n(c["ray_max_shading_opacity"])[..., 0], n(c["ray_max_far_dist"])[..., 0],
                              n(c["coarse_raycolor"]), n(c["gt"]), n(c["bg"]), n(c["edge"]), OPACITY_THRESH, far_thresh)
    return n(a), b

"""Early ray termination of render-only passes (the "cut render": include/pnerf.h pnerf_render_forward_cut): the torch-CPU
restatement on top of oracle/pyref.py and the checks that tests/test_render_cutoff_emu.py (host emulator) and
tests/test_gpu_render_cutoff.py (device) share.

Restatement: the full pyref.aggregate / ray_dist / ray_march; from its exclusive transmittance (``acc_transmission``) every ray's first stage
boundary j >= 1 with T(jB) < c; features zeroed from slot jB on; pyref.ray_march again.  (T in front of slot jB only depends on the slots
before it, which the staged render has shaded by then: the full render's T is the staged one's.)  A stage boundary is NEAR if
|T / c - 1| <= 1e-3 there: rounding may decide such a ray either way, so the rays the restatement itself flags as near are left out of the
shaded-set and value comparisons -- and the checks assert that they are at most 2 % of the hit rays.

Scenes: cases.build_case("small_k4") (100 rays, SR 16, K 4) and "small_k8" (144 rays, SR 24, K 8) with a constant added to
alpha_branch.0.bias (unshifted they never drop below T = 0.98)."""
import numpy as np
import torch

import editing_case as E
from cases import build_case
from oracle import pyref

BAR = E.BAR                 # the project's forward bar, 1e-4
NEAR = 1e-3
OUTPUTS = ("decoded", "weight", "ray_color", "opacity", "bg_trans", "blend_w")

# (case, bias shift, cutoff, stage): the rows checked on the CPU when the feature was specified
ROWS = [("small_k8", 600.0, 0.1, 2), ("small_k8", 600.0, 0.1, 4), ("small_k8", 600.0, 1e-3, 2), ("small_k8", 600.0, 1e-3, 4),
        ("small_k4", 600.0, 0.1, 2), ("small_k4", 600.0, 0.1, 4), ("small_k4", 600.0, 1e-3, 2), ("small_k4", 600.0, 1e-3, 4),
        ("small_k8", 150.0, 0.5, 2)]


def shifted_case(name, shift):
    opt, xyz, attrs, inp, mlp = build_case(name)
    mlp = dict(mlp)
    mlp["alpha_branch.0.bias"] = mlp["alpha_branch.0.bias"] + float(shift)
    return opt, xyz, attrs, inp, mlp


_FULL = {}


def full_render(name, shift, framed=False, inp=None, key=None):
    """the uncut oracle render of a shifted case, computed once per key and shared; callers leave it unchanged"""
    key = (name, float(shift), bool(framed)) if key is None else key
    if key not in _FULL:
        case = shifted_case(name, shift)
        opt, xyz, attrs, inp0, mlp = case
        inp = inp0 if inp is None else inp
        points = dict(xyz=xyz, **attrs)
        frames = E.case_frames(name) if framed else None
        with torch.no_grad():
            q = pyref.query(opt, xyz, inp)
            nb = pyref.gather_neighbors(points, q["sample_pidx"], inp["camrotc2w"][0], inp["campos"][0])
            if framed:
                feats, ray_valid, w, _ = E.aggregate_frames(opt, mlp, nb, q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"],
                                                            E.gather_frames(frames, q["sample_pidx"]))
            else:
                feats, ray_valid, w, _ = pyref.aggregate(opt, mlp, nb, q["sample_loc"], q["sample_loc_w"], q["sample_ray_dirs"])
            rd = pyref.ray_dist(opt, q["sample_loc"], ray_valid)
            color, _, opacity, acc, bw, bg_t = pyref.ray_march(rd, ray_valid, feats, inp["bg_color"])
        _FULL[key] = dict(case=(opt, xyz, attrs, inp, mlp), frames=frames, q=q, feats=feats, ray_valid=ray_valid, weight=w, rd=rd, ray_color=color[0],
                          opacity=opacity[0], acc=acc[0], blend_w=bw[0, ..., 0], bg_trans=bg_t[0, :, 0], ray_mask=q["ray_mask"])
    return _FULL[key]


def cut_of(full, c, B):
    """the restatement's cut render of ``full`` = full_render(...): dict over the R'' hit rays"""
    feats, ray_valid, acc = full["feats"], full["ray_valid"], full["acc"]
    Rh, SR = acc.shape
    B = min(int(B), SR)
    bounds = torch.arange(B, SR, B)                                         # the slots jB, j >= 1
    cut_slot = torch.full((Rh,), SR, dtype=torch.long)
    near = torch.zeros(Rh, dtype=torch.bool)
    if bounds.numel():
        Tb = acc[:, bounds]                                                 # [R'', stages - 1]
        below = Tb < c
        first = torch.where(below.any(-1), below.float().argmax(-1), torch.full((Rh,), bounds.numel(), dtype=torch.long))
        cut_slot = torch.where(below.any(-1), bounds[first.clamp(max=bounds.numel() - 1)], cut_slot)
        relevant = torch.arange(bounds.numel())[None] <= first[:, None]     # the boundaries the ray meets while alive, its last one included
        near = ((Tb / c - 1).abs() <= NEAR).logical_and(relevant).any(-1)
    keep = torch.arange(SR)[None] < cut_slot[:, None]
    with torch.no_grad():
        fc = feats * keep[None, ..., None].to(feats.dtype)
        color, _, opacity, _, bw, bg_t = pyref.ray_march(full["rd"], ray_valid, fc, full["case"][3]["bg_color"])
    shaded = ray_valid[0] & keep
    return dict(decoded=fc[0], weight=full["weight"][0] * shaded[..., None].to(feats.dtype), ray_color=color[0], opacity=opacity[0], blend_w=bw[0, ..., 0],
                bg_trans=bg_t[0, :, 0], shaded=shaded, near=near, n_shaded=int(shaded.sum()), rays_cut=int((ray_valid[0] & ~keep).any(-1).sum()))


# ------------------------------------------------------------------------------------------------- the fused model on ``dev``
def build_model(case, dev, frames=None):
    from pointnerf_amd.neural_points import NeuralPoints
    from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
    from pointnerf_amd.point_aggregators import PointAggregator
    opt, xyz, attrs, inp, mlp = case
    dev = torch.device(dev)
    agg = PointAggregator(opt).to(dev)
    agg.load_state_dict(mlp)
    agg.flatten_()
    npnt = NeuralPoints(32, xyz.shape[0], opt, dev)
    a = {k: v.to(dev) for k, v in attrs.items()}
    npnt.editing_set_points(xyz.to(dev), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"],
                            Rw2c=None if frames is None else frames.to(dev))
    model = NeuralPointsRayMarching(aggregator=agg, neural_points=npnt, opt=opt)
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return model, d


def dense_render(model, d):
    """the six dense outputs [R, ...] of one no-grad render_dense, the query's dict and the step's stats"""
    with torch.no_grad():
        t = model.render_dense(d["campos"], d["raydir"], d["camrotc2w"], d["near"], d["far"], d["bg_color"])
    out = dict(ray_color=t[0], opacity=t[1], bg_trans=t[2], blend_w=t[3], decoded=t[4], weight=t[5])
    return {k: v.detach() for k, v in out.items()}, t[7], model.last_stats


def cut_render(case, dev, c, B, frames=None, model=None):
    if model is None:
        model, d = build_model(case, dev, frames)
    else:
        model, d = model
    model.transmittance_cutoff, model.cutoff_stage = c, B
    return dense_render(model, d)


def _hit_rows(out, dense):
    hit = (dense["ray_hit"] > 0).cpu()
    return {k: v.cpu()[hit] for k, v in out.items()}, hit


def compare(got, stats, ref, full, c, tag=""):
    """assertions 1-3 for one cut render: ``got`` = the device / emulator outputs on the hit rays, ``ref`` = cut_of(full, c, B)"""
    Rh = ref["near"].numel()
    n_near = int(ref["near"].sum())
    assert n_near <= 0.02 * Rh, (tag, n_near, Rh)
    ok = ~ref["near"]
    # 1. the shaded set: the counters, and the zero pattern of opacity / decoded
    shaded = (got["decoded"] != 0).any(-1)
    valid = full["ray_valid"][0]
    assert stats["n_shaded_samples"] == int(shaded.sum()), (tag, stats["n_shaded_samples"], int(shaded.sum()))
    assert stats["rays_cut"] == int((valid & ~shaded).any(-1).sum()), tag
    if n_near == 0:
        assert stats["n_shaded_samples"] == ref["n_shaded"] and stats["rays_cut"] == ref["rays_cut"], (tag, dict(stats), ref["n_shaded"], ref["rays_cut"])
    assert torch.equal(shaded[ok], ref["shaded"][ok]), tag
    assert torch.equal((got["opacity"] > 0)[ok], (ref["opacity"] > 0)[ok]) and torch.equal((ref["opacity"] > 0)[ok], ref["shaded"][ok]), tag
    assert torch.equal((got["weight"] != 0).any(-1)[ok], ref["shaded"][ok]) and torch.equal((got["blend_w"] != 0)[ok], (ref["blend_w"] != 0)[ok]), tag
    # 2. values
    e = {k: float((got[k][ok] - ref[k][ok]).abs().max()) for k in ("opacity", "blend_w", "ray_color", "bg_trans", "weight")}
    e["rgb"] = float((got["decoded"][ok][..., 1:] - ref["decoded"][ok][..., 1:]).abs().max())
    sg, sr = got["decoded"][ok][..., 0], ref["decoded"][ok][..., 0]
    e["sigma_rel"] = float(((sg - sr).abs() / sr.abs().clamp(min=1.0)).max())
    # 3. the analytic bound against the FULL render, every hit ray
    change = float((got["ray_color"] - full["ray_color"]).abs().max())
    print(tag, "shaded %d / %d, rays cut %d / %d, near %d; errors %s; colour change vs full %.3g (bound %.3g)"
          % (stats["n_shaded_samples"], int(valid.sum()), stats["rays_cut"], Rh, n_near, {k: "%.2e" % v for k, v in e.items()}, change, 1.002 * c))
    assert all(v <= BAR for v in e.values()), (tag, e)
    assert change <= 1.002 * c + BAR, (tag, change)
    return e, change


def check_row(name, shift, c, B, dev):
    full = full_render(name, shift)
    ref = cut_of(full, c, B)
    out, dense, stats = cut_render(full["case"], dev, c, B)
    assert torch.equal((dense["ray_hit"] > 0).cpu()[None].to(torch.int8), full["ray_mask"])
    got, _ = _hit_rows(out, dense)
    return compare(got, stats, ref, full, c, "%s +%g c=%g B=%d:" % (name, shift, c, B)), ref


def check_terminates(ref, at_least):
    """the row really cuts: guards the scene, not the code"""
    assert ref["rays_cut"] >= at_least, ref["rays_cut"]


def check_bitwise_identities(name, shift, dev):
    """assertion 4: c = 0 against a model that has never heard of the option; one stage (B >= SR) with c > 0 against the uncut render; two cut
    renders of the same inputs"""
    import gpu_util
    case = shifted_case(name, shift)
    SR = int(case[0].SR)
    _, base, _ = gpu_util.hip_render(*case, train=False)             # pnerf_render_forward itself: the entry point that has never heard of the option
    assert float(base["decoded"].abs().max()) > 0
    untouched, _, st0 = dense_render(*build_model(case, dev))        # a model whose two attributes nobody has set
    zero, _, st = cut_render(case, dev, 0.0, 4)
    for k in OUTPUTS:
        assert torch.equal(base[k], untouched[k]) and torch.equal(base[k], zero[k]), ("c = 0", k)
    assert st["n_shaded_samples"] == st0["n_shaded_samples"] == st0["n_valid_samples"] and st["rays_cut"] == 0
    for B in (SR, SR + 7):
        one, _, st = cut_render(case, dev, 0.1, B)
        for k in OUTPUTS:
            assert torch.equal(base[k], one[k]), ("one stage", B, k)
        assert st["n_shaded_samples"] == st["n_valid_samples"] and st["rays_cut"] == 0
    model = build_model(case, dev)
    a, _, sa = cut_render(case, dev, 0.1, 2, model=model)
    b, _, sb = cut_render(case, dev, 0.1, 2, model=model)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), ("repeat", k)
    assert sa["n_shaded_samples"] == sb["n_shaded_samples"] < sa["n_valid_samples"] and sa["rays_cut"] == sb["rays_cut"] > 0


def check_no_termination(name, dev):
    """assertion 5: shift 0, c = 1e-3, B = 4: nothing ends early; every output within the bar of the UNCUT oracle render.  Returns whether the
    staged render is also bit-identical to the uncut device render (recorded in DESIGN.md 4.6, not asserted: the tile composition differs)"""
    full = full_render(name, 0.0)
    assert float(full["bg_trans"].min()) > 0.9
    out, dense, stats = cut_render(full["case"], dev, 1e-3, 4)
    got, _ = _hit_rows(out, dense)
    assert stats["rays_cut"] == 0 and stats["n_shaded_samples"] == stats["n_valid_samples"] == int(full["ray_valid"].sum())
    ref = dict(decoded=full["feats"][0], weight=full["weight"][0], ray_color=full["ray_color"], opacity=full["opacity"], bg_trans=full["bg_trans"],
               blend_w=full["blend_w"])
    e = {k: float((got[k] - ref[k]).abs().max()) for k in OUTPUTS}
    assert all(v <= BAR for v in e.values()), e
    uncut, _, _ = cut_render(full["case"], dev, 0.0, 4)
    same = all(torch.equal(out[k], uncut[k]) for k in OUTPUTS)
    print(name, "no termination: errors", e, "; bit-identical to the uncut render:", same)
    return same


def check_frames(dev):
    """assertion 6: one editing case through the cut route: small_k8 +600 with 3-part frames, c = 0.1, B = 2, against the restatement built on
    editing_case.aggregate_frames"""
    name, shift, c, B = "small_k8", 600.0, 0.1, 2
    full = full_render(name, shift, framed=True)
    ref = cut_of(full, c, B)
    model, d = E.build_model(name, dev, full["frames"])
    with torch.no_grad():
        model.aggregator.alpha_branch[0].bias.add_(shift)
    out, dense, stats = cut_render(None, dev, c, B, model=(model, d))
    got, _ = _hit_rows(out, dense)
    compare(got, stats, ref, full, c, "frames %s +%g c=%g B=%d:" % (name, shift, c, B))
    check_terminates(ref, 100)


def check_refusals(dev):
    """assertion 7: a training forward and opt.prob = 1 each raise, naming the option"""
    import pytest
    case = shifted_case("small_k4", 600.0)
    model, d = build_model(case, dev)
    model.transmittance_cutoff = 0.1
    with pytest.raises(NotImplementedError, match="transmittance_cutoff"):
        model(**d)                                                   # gradients enabled: a training forward
    with pytest.raises(NotImplementedError, match="transmittance_cutoff"), torch.no_grad():
        model.render_dense(d["campos"], d["raydir"], d["camrotc2w"], d["near"], d["far"], d["bg_color"], train=True)
    case[0].prob = 1
    try:
        with pytest.raises(NotImplementedError, match="transmittance_cutoff"), torch.no_grad():
            model(**d)
    finally:
        case[0].prob = 0
    model.fused_probe = True
    with pytest.raises(NotImplementedError, match="transmittance_cutoff"), torch.no_grad():
        model(**d)
    model.fused_probe = False
    for bad in (1.0, -0.1, 1.5):
        model.transmittance_cutoff = bad
        with pytest.raises(ValueError, match="transmittance_cutoff"), torch.no_grad():
            model(**d)
    model.transmittance_cutoff, model.cutoff_stage = 0.1, 0
    with pytest.raises(ValueError, match="cutoff_stage"), torch.no_grad():
        model(**d)
    model.cutoff_stage = 4
    with torch.no_grad():
        out = model(**d)                                             # the render-only pass itself is served
    assert out["coarse_raycolor"].shape[1] == model.last_stats["rays_hit"] and model.last_stats["rays_cut"] > 0


IMAGE = dict(name="small_k8", shift=600.0, size=24, x0=404, y0=388, c=0.1, B=4, chunk=200)      # (x0 = 388 centres the block on the cloud: no ray misses)


def check_render_image(dev):
    """assertion 8: eval_loop.render_image of a 24 x 24 view in three chunks with c = 0.1, B = 4: every channel within 1.002 c + 1e-4 of the
    oracle's uncut image, the hit mask equal, the model's setting restored"""
    from pointnerf_amd import eval_loop, scenes
    I = IMAGE
    case = shifted_case(I["name"], I["shift"])
    opt, xyz, attrs, _, mlp = case
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=I["x0"], y0=I["y0"], size=I["size"]))
    intr = inp["intrinsic"][0].clone()
    intr[0, 2] -= float(I["x0"]); intr[1, 2] -= float(I["y0"])
    h = w = I["size"]
    inp = dict(inp)
    inp["raydir"] = eval_loop.rays_from_pixels(eval_loop.pixel_grid(h, w, torch.device("cpu")), intr, inp["camrotc2w"])
    full = full_render(I["name"], I["shift"], inp=inp, key="image")
    hit_ref = full["ray_mask"][0] > 0
    assert 50 < int(hit_ref.sum()) < hit_ref.numel() - 20, int(hit_ref.sum())          # rays that hit and rays that miss
    image_ref = pyref.fill_invalid(dict(ray_mask=full["ray_mask"], coarse_raycolor=full["ray_color"][None], coarse_is_background=full["bg_trans"][None, :, None],
                                        coarse_point_opacity=full["opacity"][None]), inp)["coarse_raycolor"][0]
    model, d = build_model((opt, xyz, attrs, inp, mlp), dev)
    model.transmittance_cutoff, model.cutoff_stage = 0.0, 7
    assert h * w > 2 * I["chunk"]
    img, hit = eval_loop.render_image(model, d["campos"], d["camrotc2w"], intr, h, w, d["near"], d["far"], d["bg_color"], chunk=I["chunk"],
                                      transmittance_cutoff=I["c"], cutoff_stage=I["B"])
    assert model.last_stats["rays_cut"] > 0                                            # the last chunk went through the cut route
    assert (model.transmittance_cutoff, model.cutoff_stage) == (0.0, 7)
    assert torch.equal(hit.cpu(), hit_ref)
    change = float((img.cpu().reshape(-1, 3) - image_ref).abs().max())
    print("render_image: colour change vs the uncut oracle image %.3g (bound %.3g)" % (change, 1.002 * I["c"]))
    assert 1e-3 < change <= 1.002 * I["c"] + BAR, change


def check_arithmetic_option(dev, option):
    """the cut route under the other inference arithmetics ("products2": pnerf_set_inference_products(2); "e4m3": bit 0 of
    pnerf_set_cross_terms_where): the launches are the uncut render's, so ONE stage equals the uncut render of the same mode bit for bit,
    and the analytic bound holds"""
    from pointnerf_amd import ops
    full = full_render("small_k4", 600.0)
    old = ops.set_inference_products(2) if option == "products2" else ops.set_cross_terms(8, where=5)
    try:
        base, _, _ = cut_render(full["case"], dev, 0.0, 4)
        one, _, _ = cut_render(full["case"], dev, 0.1, 64)
        for k in OUTPUTS:
            assert torch.equal(base[k], one[k]), k
        out, dense, stats = cut_render(full["case"], dev, 0.1, 2)
        got, _ = _hit_rows(out, dense)
        assert stats["rays_cut"] > 50 and float((got["ray_color"] - full["ray_color"]).abs().max()) <= 1.002 * 0.1 + BAR
    finally:
        if option == "products2":
            ops.set_inference_products(old)
        else:
            ops.set_cross_terms(old[0], where=old[1])


def check_entry_point_arguments(dev):
    """pnerf_render_forward_cut: cutoff outside [0, 1) / stage_samples < 1 -> PNERF_E_INVAL; cutoff == 0 runs pnerf_render_forward's body"""
    import ctypes
    import pytest
    import gpu_util
    from pointnerf_amd import _lib as L, ops
    opt, xyz, attrs, inp, mlp = shifted_case("small_k4", 600.0)
    dense, fwd, ctx = gpu_util.hip_render(opt, xyz, attrs, inp, mlp, train=False)
    args = (ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"])
    zero = ops.render_forward_cut(*args, 0.0, 4)
    for k in OUTPUTS:
        assert torch.equal(zero[k], fwd[k]), k
    assert zero["cut_counters"].cpu().tolist() == [ctx["n_valid"], 0, 0, 0]
    cut = ops.render_forward_cut(*args, 0.1, 2)
    n_shaded, rays_cut, z2, z3 = cut["cut_counters"].cpu().tolist()
    assert 0 < n_shaded < ctx["n_valid"] and rays_cut > 50 and z2 == z3 == 0
    st = ops.make_step(ctx["raydir"], dense, ctx["flat"], ctx["packed"], ctx["R"], opt.SR, opt.K, ctx["n_valid"])
    lib = L.lib()
    nws = lib.pnerf_agg_workspace_bytes(ctx["n_valid"], opt.K)
    ncut = lib.pnerf_render_cut_workspace_bytes(ctx["R"], opt.SR)
    assert ncut > ctx["R"] * opt.SR * 8
    ws, cws, cc = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(ncut, dtype=torch.uint8, device=dev), torch.empty(4, dtype=torch.int32, device=dev)

    def call(cutoff, stage, cut_ws=cws, cut_bytes=ncut, counters=cc):
        P = ops._ptr
        return lib.pnerf_render_forward_cut(ctypes.byref(ctx["cam"]), ctypes.byref(ctx["pts"]), ctypes.byref(st), cutoff, stage, P(cut["decoded"]), P(cut["weight"]),
                                            P(cut["ray_color"]), P(cut["opacity"]), P(cut["bg_trans"]), P(cut["blend_w"]), P(counters), P(ws), nws, P(cut_ws),
                                            cut_bytes, ops._stream())
    assert call(1.0, 4) == -1 and call(-0.5, 4) == -1 and call(float("nan"), 4) == -1 and call(0.1, 0) == -1 and call(0.1, 4, counters=None) == -1
    assert call(0.1, 4, cut_bytes=ncut - 1) == -2 and call(0.1, 4, cut_ws=None) == -2
    with pytest.raises(ValueError, match="transmittance_cutoff"):
        ops.render_forward_cut(*args, 1.0, 4)


# ------------------------------------------------------------------------------------------------- pnerf_cut_stage on synthetic arrays
STAGE_R, STAGE_C, STAGE_SEED = 37, 0.05, 7          # the seed: no stage boundary within 1e-3 of the cutoff for any (SR, B) of the tests (asserted)
STAGE_VS = 0.004


def stage_inputs(SR, seed=STAGE_SEED):
    """random neighbor counts with gaps and empty rays, sample positions along the rays (depth = z: identity camera at the origin; mostly rising
    by less than 2 vsize, some falling back -- the cummax holds, the delta becomes vsize -- and some jumping by more than 2 vsize), sigma scaled so
    that T crosses STAGE_C at slots spread over the whole ray (and never, for some rays)"""
    rng = np.random.default_rng(seed + SR)
    R = STAGE_R
    nn = (rng.random((R, SR)) < 0.7).astype(np.int32) * rng.integers(1, 9, size=(R, SR)).astype(np.int32)
    nn[rng.random(R) < 0.12] = 0                                              # empty rays
    nn[3, : SR // 2] = 0                                                      # a ray whose first half is empty
    hit = (nn.sum(1) > 0).astype(np.int32)
    step = rng.uniform(0.25, 1.5, size=(R, SR)) * STAGE_VS
    kind = rng.random((R, SR))
    step[kind < 0.10] = -0.5 * STAGE_VS                                       # falls back behind the running maximum
    step[kind > 0.93] = 3.1 * STAGE_VS                                        # a gap of more than 2 vsize
    z = (2.0 + np.cumsum(step, axis=1)).astype(np.float32)
    loc = np.stack([rng.uniform(-1, 1, size=(R, SR)), rng.uniform(-1, 1, size=(R, SR)), z], -1).astype(np.float32)
    cross = np.maximum(rng.uniform(0.05, 1.3, size=(R, 1)) * SR, 3.0)         # where the ray should reach T = c (beyond SR: never)
    sigma = -np.log(STAGE_C) / (cross * 0.7 * STAGE_VS) * rng.uniform(0.5, 1.5, size=(R, SR))
    sigma = np.minimum(sigma, 1.2 / (1.5 * STAGE_VS)).astype(np.float32)      # every factor u >= 0.3: its fp32 rounding stays ~2e-7 relative
    decoded = np.concatenate([sigma[..., None], rng.random((R, SR, 3), dtype=np.float32)], -1).astype(np.float32)
    decoded[nn == 0] = 0.0
    return loc, nn, hit, decoded


def stage_restatement(loc, nn, hit, decoded, c, B):
    """float64 numpy: per stage (T [R], alive [R] in the library's coding, flags [R,SR]) and whether a boundary a ray meets is near"""
    R, SR = nn.shape
    B = min(B, SR)
    z = loc[..., 2].astype(np.float64)
    cm = np.maximum.accumulate(z, axis=1)
    d = np.concatenate([cm[:, 1:] - cm[:, :-1], np.full((R, 1), np.float64(np.float32(STAGE_VS)))], 1)
    vs = np.float64(np.float32(STAGE_VS))
    d = np.where((d < 1e-8) | (d > 2 * vs), vs, d)
    valid = nn > 0
    op = 1 - np.exp(-np.where(valid, decoded[..., 0].astype(np.float64), 0.0) * np.where(valid, d, 0.0))
    u = 1 - op + 1e-10
    Tx = np.concatenate([np.ones((R, 1)), np.cumprod(u, axis=1)[:, :-1]], 1)           # exclusive
    alive = (hit > 0).astype(np.int32)
    T = np.ones(R)
    near = False
    stages = []
    for j in range((SR + B - 1) // B):
        if j > 0:
            for r in range(R):
                if alive[r] == 1:
                    T[r] = Tx[r, j * B]
                    near = near or abs(T[r] / c - 1) <= NEAR
                    if not T[r] >= c:
                        alive[r] = 2 if valid[r, j * B:].any() else 0
        flags = np.zeros((R, SR), np.int32)
        flags[:, j * B:(j + 1) * B] = (valid[:, j * B:(j + 1) * B] & (alive[:, None] == 1)).astype(np.int32)
        stages.append((T.copy(), alive.copy(), flags))
    return stages, near


def check_cut_stage(SR, B, dev):
    """assertion 9: flags, list, count and alive state equal, the carried T within 1e-5 relative (an fp32 product of at most 128 factors)"""
    from pointnerf_amd import ops
    loc, nn, hit, decoded = stage_inputs(SR)
    stages, near = stage_restatement(loc, nn, hit, decoded, STAGE_C, B)
    assert not near, "the generator's seed puts a stage boundary within 1e-3 of the cutoff"
    died = [int((a != 1).sum()) for _, a, _ in stages]
    if len(stages) > 1:
        assert died[-1] - died[0] >= 5 and int((stages[-1][1] == 1).sum()) >= 3, died         # rays end at stage boundaries, and some never do
    cam = ops.make_camera([0, 0, 0], np.eye(3), STAGE_VS, 1, bg=None)
    t = lambda a: torch.from_numpy(a).to(dev)
    loc_t, nn_t, hit_t, dec_t = t(loc), t(nn), t(hit), t(decoded)
    state = None
    for j, (T, alive, flags) in enumerate(stages):
        state = ops.cut_stage(cam, loc_t, nn_t, hit_t, dec_t, STAGE_C, B, j, state)
        got = {k: v.cpu().numpy() for k, v in state.items()}
        assert np.array_equal(got["alive"], alive), (SR, B, j)
        assert np.array_equal(got["flags"], flags), (SR, B, j)
        n = int(flags.sum())
        assert got["counters"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
        assert np.array_equal(got["list"][:n], np.flatnonzero(flags.reshape(-1)))
        rel = np.abs(got["trans"].astype(np.float64) / T - 1)
        assert rel.max() <= 1e-5, (SR, B, j, rel.max())
    assert _stage_refused(cam, loc_t, nn_t, hit_t, dec_t, B, len(stages), state)


def _stage_refused(cam, loc_t, nn_t, hit_t, dec_t, B, stage, state):
    """a stage beyond the last one, and a cutoff outside (0, 1), are PNERF_E_INVAL"""
    import pytest
    from pointnerf_amd import ops
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
        ops.cut_stage(cam, loc_t, nn_t, hit_t, dec_t, STAGE_C, B, stage, state)
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
        ops.cut_stage(cam, loc_t, nn_t, hit_t, dec_t, 0.0, B, 0, state)
    return True

"""Per-ray depth and opacity maps of render-only passes (include/pnerf.h pnerf_ray_geometry / pnerf_geometry_canvas): the
float64 restatement and the checks that tests/test_ray_geometry_emu.py (host emulator) and tests/test_gpu_ray_geometry.py (device) share.

Restatement (per ray, over the slots s): acc = sum bw_s; depth_sum = sum over the valid s of bw_s z_s; depth = depth_sum / (acc + 1e-6);
T_s = prod_{j <= s} (1 - op_j + 1e-10); median_slot = the lowest valid s with T_s < 0.5 (-1: none), median_depth = z there (0: none).  It
is fed what the kernel is fed -- opacity and blend weight as the renderer (or its float64 restatement, cast to fp32) left them -- so what is
measured is the kernel's own arithmetic.  A ray is NEAR if some valid slot has |T_s / 0.5 - 1| <= 1e-3 in float64: rounding may put its
crossing one slot either way, so near rays are left out of the slot / median comparisons, and the checks bound how many there may be."""
import ctypes

import numpy as np
import pytest
import torch

import cutoff_case as C
import editing_case as E

BAR = C.BAR                  # the project's forward bar, 1e-4
NEAR = 1e-3
KERNEL_SR = (16, 24, 64, 65, 80, 128)        # one chunk, the chunk boundary (64 / 65), a partial second chunk, two full chunks
# the keys of a forward with ray_geometry off (build_case's options: zero-one regulariser on conf_coefficient, no probe outputs)
PARENT_KEYS = ["_hit_index", "blend_weight", "coarse_is_background", "coarse_point_opacity", "coarse_raycolor", "conf_coefficient", "queried_shading",
               "ray_mask", "weight"]
GEOMETRY_KEYS = ("coarse_depth", "coarse_median_depth", "coarse_acc")


def restate(z, valid, op, bw):
    """float64 numpy, [R, SR] each -> dict(acc, depth_sum, depth, median_slot, median_depth, near [R] bool)"""
    z, op, bw = (np.asarray(a, dtype=np.float64) for a in (z, op, bw))
    valid = np.asarray(valid, dtype=bool)
    acc = bw.sum(1)
    depth_sum = np.where(valid, bw * np.where(valid, z, 0.0), 0.0).sum(1)
    Tin = np.cumprod(1 - op + 1e-10, axis=1)
    below = valid & (Tin < 0.5)
    slot = np.where(below.any(1), below.argmax(1), -1)
    zv = np.where(valid, z, 0.0)
    median = np.where(slot >= 0, zv[np.arange(z.shape[0]), np.maximum(slot, 0)], 0.0)
    near = (valid & (np.abs(Tin / 0.5 - 1) <= NEAR)).any(1)
    return dict(acc=acc, depth_sum=depth_sum, depth=depth_sum / (acc + 1e-6), median_slot=slot, median_depth=median, near=near)


# ------------------------------------------------------------------------------------------------- 1. the kernel on synthetic arrays
def stage_opacity(loc, nn, decoded):
    """opacity and blend weight of cutoff_case.stage_inputs in float64, formed exactly as cutoff_case.stage_restatement forms them"""
    R, SR = nn.shape
    z = loc[..., 2].astype(np.float64)
    cm = np.maximum.accumulate(z, axis=1)
    vs = np.float64(np.float32(C.STAGE_VS))
    d = np.concatenate([cm[:, 1:] - cm[:, :-1], np.full((R, 1), vs)], 1)
    d = np.where((d < 1e-8) | (d > 2 * vs), vs, d)
    valid = nn > 0
    op = 1 - np.exp(-np.where(valid, decoded[..., 0].astype(np.float64), 0.0) * np.where(valid, d, 0.0))
    u = 1 - op + 1e-10
    Tx = np.concatenate([np.ones((R, 1)), np.cumprod(u, axis=1)[:, :-1]], 1)           # exclusive
    return op, op * Tx


def check_kernel(SR, dev, sigma_scale=1.0):
    """``sigma_scale`` 1: every hit ray crosses T = 0.5; 0.02: none does (the -1 / 0 branch)"""
    from pointnerf_amd import ops
    loc, nn, hit, decoded = C.stage_inputs(SR)
    decoded = decoded.copy()
    decoded[..., 0] *= np.float32(sigma_scale)
    op64, bw64 = stage_opacity(loc, nn, decoded)
    op, bw = op64.astype(np.float32), bw64.astype(np.float32)          # what the kernel is handed ...
    ref = restate(loc[..., 2], nn > 0, op, bw)                           # ... and the restatement too
    hitb = hit > 0
    crosses = ref["median_slot"][hitb] >= 0
    if sigma_scale == 1.0:
        assert crosses.all(), "the generator: a hit ray that never crosses"
        if SR == 128:
            assert ref["median_slot"].max() >= 64                        # crossings in both chunks
    else:
        assert not crosses.any(), "the generator: a ray crosses at the small scale"
    n_near = int(ref["near"][hitb].sum())
    assert n_near <= 1, (SR, n_near)                                     # a condition on the generator's seed, not a measurement
    # rows that must not be read are poisoned: positions of empty slots, opacity / blend weight of the rays that missed
    loc_in, op_in, bw_in = loc.copy(), op.copy(), bw.copy()
    loc_in[nn == 0] = np.nan
    op_in[~hitb] = np.nan
    bw_in[~hitb] = np.nan
    cam = ops.make_camera([0, 0, 0], np.eye(3), C.STAGE_VS, 1, bg=None)
    t = lambda a: torch.from_numpy(a).to(dev)
    args = (cam, t(loc_in), t(nn), t(hit), t(op_in), t(bw_in))
    got = {k: v.cpu().numpy() for k, v in ops.ray_geometry(*args).items() if k in ops.RAY_GEOMETRY_KEYS}
    again = {k: v.cpu().numpy() for k, v in ops.ray_geometry(*args).items() if k in ops.RAY_GEOMETRY_KEYS}
    assert sorted(got) == sorted(["acc", "depth_sum", "depth", "median_depth", "median_slot"])
    for k in got:
        assert got[k].shape == (C.STAGE_R,) and np.array_equal(got[k], again[k]), ("two calls", k)
        assert got[k].dtype == (np.int32 if k == "median_slot" else np.float32)
    # rays that missed: zeros and -1
    assert hitb.sum() < C.STAGE_R
    for k in ("acc", "depth_sum", "depth", "median_depth"):
        assert np.array_equal(got[k][~hitb], np.zeros(int((~hitb).sum()), np.float32)), k
    assert (got["median_slot"][~hitb] == -1).all()
    e = dict(acc=np.abs(got["acc"] - ref["acc"])[hitb].max(), depth_sum=np.abs(got["depth_sum"] - ref["depth_sum"])[hitb].max(),
             depth_rel=(np.abs(got["depth"] - ref["depth"])[hitb] / np.abs(ref["depth"][hitb])).max())
    ok = hitb & ~ref["near"]
    print("SR %d scale %g: errors %s, near %d, slots up to %d" % (SR, sigma_scale, {k: "%.2e" % v for k, v in e.items()}, n_near, got["median_slot"].max()))
    assert np.array_equal(got["median_slot"][ok], ref["median_slot"][ok]), SR
    # median_depth: the bits of fp32(z) at the slot the kernel reports (every hit ray, the near ones too); 0 without a crossing
    s = got["median_slot"]
    assert ((s >= -1) & (s < SR)).all() and (nn[np.arange(C.STAGE_R), np.maximum(s, 0)][s >= 0] > 0).all()
    want = np.where(s >= 0, loc[np.arange(C.STAGE_R), np.maximum(s, 0), 2], np.float32(0)).astype(np.float32)
    assert np.array_equal(got["median_depth"].view(np.int32), want.view(np.int32)), SR
    assert e["acc"] <= 1e-5 and e["depth_sum"] <= 1e-5 and e["depth_rel"] <= 1e-5, (SR, e)       # an fp32 sum / product of at most 128 terms
    return e


def check_entry_refusals(dev):
    """pnerf_ray_geometry: SR = 0 and a null output are PNERF_E_INVAL; R = 0 is a no-op"""
    from pointnerf_amd import _lib as L, ops
    loc, nn, hit, decoded = C.stage_inputs(16)
    op64, bw64 = stage_opacity(loc, nn, decoded)
    cam = ops.make_camera([0, 0, 0], np.eye(3), C.STAGE_VS, 1, bg=None)
    t = lambda a: torch.from_numpy(a).to(dev)
    ins = [t(loc), t(nn), t(hit), t(op64.astype(np.float32)), t(bw64.astype(np.float32))]
    outs = [torch.empty(C.STAGE_R, dtype=torch.int32 if i == 4 else torch.float32, device=dev) for i in range(5)]
    P = ops._ptr

    def call(R, SR, ins=ins, outs=outs):
        return L.lib().pnerf_ray_geometry(ctypes.byref(cam), *[P(x) for x in ins], R, SR, *[P(x) for x in outs], ops._stream())
    assert call(C.STAGE_R, 0) == -1 and call(-1, 16) == -1
    assert call(C.STAGE_R, 16, outs=[None] + outs[1:]) == -1 and call(C.STAGE_R, 16, outs=outs[:4] + [None]) == -1
    assert call(C.STAGE_R, 16, ins=[None] + ins[1:]) == -1
    assert call(0, 16, ins=[None] * 5, outs=[None] * 5) == 0
    assert call(C.STAGE_R, 16) == 0
    with pytest.raises(ValueError, match="opacity"):
        ops.ray_geometry(cam, ins[0], ins[1], ins[2], ins[3][:, :8].contiguous(), ins[4])
    with pytest.raises(ValueError, match="ray_hit"):
        ops.ray_geometry(cam, ins[0], ins[1], ins[2].float(), ins[3], ins[4])


# ------------------------------------------------------------------------------------------------- 2. through the model against oracle/pyref.py
def oracle_geometry(opacity, blend_w, z, valid):
    """the restatement on an oracle render's own tensors over the R'' hit rays"""
    return restate(z.double().numpy(), valid.numpy(), opacity.double().numpy(), blend_w.double().numpy())


def full_geometry(full):
    return oracle_geometry(full["opacity"], full["blend_w"], full["q"]["sample_loc"][0, ..., 2], full["ray_valid"][0])


def forward_geometry(model, d):
    with torch.no_grad():
        out = model(**d)
    return out, {k: out[k].cpu() for k in GEOMETRY_KEYS}


def compare_forward(got, ref, n_hit, tag, near_share=0.02):
    """coarse_acc / coarse_depth at the forward bar, coarse_median_depth within 1e-6 of the oracle's z at the oracle's slot off the near rays"""
    for k in GEOMETRY_KEYS:
        assert tuple(got[k].shape) == (1, n_hit, 1) and got[k].dtype == torch.float32, (tag, k, got[k].shape)
    g = {k: got[k][0, :, 0].double().numpy() for k in GEOMETRY_KEYS}
    n_near = int(ref["near"].sum())
    assert n_near <= near_share * n_hit, (tag, n_near, n_hit)
    ok = ~ref["near"]
    e = dict(acc=np.abs(g["coarse_acc"] - ref["acc"]).max(), depth=np.abs(g["coarse_depth"] - ref["depth"]).max(),
             median=np.abs(g["coarse_median_depth"] - ref["median_depth"])[ok].max())
    print(tag, "errors %s; near %d of %d; rays that cross %d" % ({k: "%.2e" % v for k, v in e.items()}, n_near, n_hit, int((ref["median_slot"] >= 0).sum())))
    assert e["acc"] <= BAR and e["depth"] <= BAR, (tag, e)
    assert e["median"] <= 1e-6, (tag, e)
    return e


def check_model(name, shift, dev):
    full = C.full_render(name, shift)
    ref = full_geometry(full)
    model, d = C.build_model(full["case"], dev)
    assert model.ray_geometry is False
    model.ray_geometry = True
    out, got = forward_geometry(model, d)
    n_hit = int(full["ray_mask"].sum())
    assert torch.equal(out["ray_mask"].cpu(), full["ray_mask"])
    compare_forward(got, ref, n_hit, "%s +%g:" % (name, shift))
    if shift == 0:
        assert (ref["median_slot"] == -1).all() and float(got["coarse_median_depth"].abs().max()) == 0.0        # nothing crosses: all medians 0
    else:
        assert (ref["median_slot"] >= 0).sum() >= n_hit // 2                                                     # (guards the scene)
    assert sorted(set(out) - set(GEOMETRY_KEYS) - {"_dense_geometry"}) == PARENT_KEYS
    from pointnerf_amd.neural_points_volumetric_model import fill_invalid
    hit = full["ray_mask"][0] > 0
    R = hit.numel()
    # fill_invalid: from the kernel's full-size results when the forward handed them along, else by scattering the compacted keys
    for o in (out, {k: v for k, v in out.items() if k != "_dense_geometry"}):
        filled = fill_invalid(o, d["bg_color"])
        for k in GEOMETRY_KEYS:
            f = filled[k].cpu()
            assert tuple(f.shape) == (1, R, 1)
            assert torch.equal(f[0, hit], got[k][0]) and float(f[0, ~hit].abs().sum()) == 0.0, k
        assert tuple(filled["coarse_raycolor"].shape) == (1, R, 3)


def check_unchanged(name, shift, dev):
    """attribute off: exactly the parent's keys, and the six dense outputs are pnerf_render_forward's bits"""
    import gpu_util
    case = C.shifted_case(name, shift)
    _, base, _ = gpu_util.hip_render(*case, train=False)
    model, d = C.build_model(case, dev)
    assert model.ray_geometry is False
    with torch.no_grad():
        out = model(**d)
    assert sorted(out) == PARENT_KEYS, sorted(out)
    dense, _, _ = C.dense_render(model, d)
    for k in C.OUTPUTS:
        assert torch.equal(base[k], dense[k]), k
    model.ray_geometry = True                        # ... and render_dense hands out the same bits when the maps are asked for
    dense, _, _ = C.dense_render(model, d)
    for k in C.OUTPUTS:
        assert torch.equal(base[k], dense[k]), ("ray_geometry on", k)


# ------------------------------------------------------------------------------------------------- 3. the cut route
def check_cut_route(dev):
    """small_k8 +600, c = 0.1, B = 2 against the UNCUT oracle: the mass the cut drops is below c"""
    from pointnerf_amd import ops
    name, shift, c, B = "small_k8", 600.0, 0.1, 2
    full = C.full_render(name, shift)
    ref = full_geometry(full)
    zmax = float(np.abs(np.where(full["ray_valid"][0].numpy(), full["q"]["sample_loc"][0, ..., 2].double().numpy(), 0.0)).max())
    model, d = C.build_model(full["case"], dev)
    model.transmittance_cutoff, model.cutoff_stage, model.ray_geometry = c, B, True
    out, got = forward_geometry(model, d)
    assert model.last_stats["rays_cut"] > 50                                                  # the render really took the cut route
    dn, dense, _ = C.dense_render(model, d)
    opt, inp = full["case"][0], full["case"][3]
    cam = ops.make_camera(inp["campos"][0].numpy(), inp["camrotc2w"][0].numpy(), opt.vsize[2], opt.raydist_mode_unit)
    geo = ops.ray_geometry(cam, dense["sample_loc"], dense["sample_nn"], dense["ray_hit"], dn["opacity"], dn["blend_w"])
    hit = (dense["ray_hit"] > 0).cpu()
    g = {k: geo[k].cpu()[hit] for k in ops.RAY_GEOMETRY_KEYS}
    for key, k in (("coarse_acc", "acc"), ("coarse_depth", "depth"), ("coarse_median_depth", "median_depth")):
        assert torch.equal(got[key][0, :, 0], g[k]), key                                      # the forward's keys are this launch's values
    e = dict(acc=np.abs(g["acc"].double().numpy() - ref["acc"]).max(), depth_sum=np.abs(g["depth_sum"].double().numpy() - ref["depth_sum"]).max())
    ok = ~ref["near"]
    e["median"] = np.abs(g["median_depth"].double().numpy() - ref["median_depth"])[ok].max()
    print("cut route c=%g B=%d: acc change %.3g (bound %.3g), depth_sum change %.3g (bound %.3g), median %.2e, near %d"
          % (c, B, e["acc"], c, e["depth_sum"], c * zmax, e["median"], int(ref["near"].sum())))
    assert int(ref["near"].sum()) <= 0.02 * ok.size
    assert e["acc"] <= c + BAR and e["depth_sum"] <= c * zmax + BAR, e
    assert e["median"] <= 1e-6, e                                                             # the uncut render's median, c < 0.5
    assert np.array_equal(g["median_slot"].numpy()[ok], ref["median_slot"][ok])


# ------------------------------------------------------------------------------------------------- 4. per-point frames
def check_frames(dev, name="small_k8"):
    case, frames, r = E.reference(name)
    ref = oracle_geometry(r["coarse_point_opacity"][0], r["blend_weight"][0, ..., 0], r["query"]["sample_loc"][0, ..., 2], r["ray_valid"][0])
    model, d = E.build_model(name, dev, frames)
    model.ray_geometry = True
    out, got = forward_geometry(model, d)
    assert torch.equal(out["ray_mask"].cpu(), r["ray_mask"])
    compare_forward(got, ref, int(r["ray_mask"].sum()), "frames %s:" % name)


# ------------------------------------------------------------------------------------------------- 5. refusals
def check_refusals(dev):
    case = C.shifted_case("small_k4", 600.0)
    model, d = C.build_model(case, dev)
    model.ray_geometry = True
    with pytest.raises(NotImplementedError, match="ray_geometry"):
        model(**d)                                                   # gradients enabled: a training forward
    with pytest.raises(NotImplementedError, match="ray_geometry"), torch.no_grad():
        model.render_dense(d["campos"], d["raydir"], d["camrotc2w"], d["near"], d["far"], d["bg_color"], train=True)
    case[0].prob = 1
    try:
        with pytest.raises(NotImplementedError, match="ray_geometry"), torch.no_grad():
            model(**d)
    finally:
        case[0].prob = 0
    model.fused_probe = True
    with pytest.raises(NotImplementedError, match="ray_geometry"), torch.no_grad():
        model(**d)
    model.fused_probe = False
    with torch.no_grad():
        out = model(**d)                                             # the render-only pass itself is served
    assert all(k in out for k in GEOMETRY_KEYS)
    from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
    with pytest.raises(NotImplementedError, match="undefined ray_ts"):
        NeuralPointsRayMarching(is_compute_depth=True, opt=case[0])
    case[0].ray_geometry = True                                      # opt.ray_geometry is the initial value
    try:
        assert NeuralPointsRayMarching(opt=case[0]).ray_geometry is True
    finally:
        del case[0].ray_geometry
    assert NeuralPointsRayMarching(opt=case[0]).ray_geometry is False


# ------------------------------------------------------------------------------------------------- 6. render_image(geometry=True)
def check_render_image(dev):
    from pointnerf_amd import eval_loop, ops, scenes
    from oracle import pyref
    I = C.IMAGE
    opt, xyz, attrs, _, mlp = C.shifted_case(I["name"], I["shift"])
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=I["x0"], y0=I["y0"], size=I["size"]))
    intr = inp["intrinsic"][0].clone()
    intr[0, 2] -= float(I["x0"]); intr[1, 2] -= float(I["y0"])
    h = w = I["size"]
    inp = dict(inp)
    inp["raydir"] = eval_loop.rays_from_pixels(eval_loop.pixel_grid(h, w, torch.device("cpu")), intr, inp["camrotc2w"])
    full = C.full_render(I["name"], I["shift"], inp=inp, key="image")          # (the cut render's image test shares it)
    ref = full_geometry(full)
    hit_ref = full["ray_mask"][0] > 0
    n_hit = int(hit_ref.sum())
    assert 50 < n_hit < hit_ref.numel() - 20
    model, d = C.build_model((opt, xyz, attrs, inp, mlp), dev)
    assert h * w > 2 * I["chunk"]
    a = (model, d["campos"], d["camrotc2w"], intr, h, w, d["near"], d["far"], d["bg_color"])
    plain = eval_loop.render_image(*a, chunk=I["chunk"])
    assert len(plain) == 2
    img, hit, maps = eval_loop.render_image(*a, chunk=I["chunk"], geometry=True)
    assert model.ray_geometry is False                                          # restored
    assert torch.equal(img, plain[0]) and torch.equal(hit, plain[1]) and torch.equal(hit.cpu(), hit_ref)
    assert sorted(maps) == ["acc", "depth", "median_depth"]
    n_near = int(ref["near"].sum())
    assert n_near <= 0.02 * n_hit
    e = {}
    for k in ("acc", "depth", "median_depth"):
        m = maps[k].cpu()
        assert tuple(m.shape) == (h, w) and m.dtype == torch.float32
        want = torch.zeros(h * w, dtype=torch.float64)
        want[hit_ref] = torch.from_numpy(ref[k])
        keep = torch.ones(h * w, dtype=torch.bool)
        if k == "median_depth":
            keep[hit_ref] = torch.from_numpy(~ref["near"])
        e[k] = float((m.reshape(-1).double() - want).abs()[keep].max())
        if k != "median_depth":
            assert torch.equal(m.reshape(-1) == 0, ~hit_ref), k                 # zero exactly where the ray missed
        else:
            assert float(m.reshape(-1)[~hit_ref].abs().sum()) == 0.0
    print("render_image maps: errors %s, near %d of %d" % ({k: "%.2e" % v for k, v in e.items()}, n_near, n_hit))
    assert all(v <= BAR for v in e.values()), e
    # depth_points: one row per hit pixel, campos + depth * raydir
    pts = eval_loop.depth_points(maps["depth"], d["campos"], d["camrotc2w"], intr)
    assert tuple(pts.shape) == (n_hit, 3)
    depth = maps["depth"].cpu().reshape(-1)
    want = inp["campos"].reshape(1, 3) + depth[hit_ref][:, None] * inp["raydir"][0][hit_ref]
    assert float((pts.cpu() - want).abs().max()) <= BAR
    check_canvas(dev, h, w)


def check_canvas(dev, h=24, w=24):
    """ops.geometry_canvas alone: values at their pixels, 0 for a masked ray, no other pixel touched; a pixel outside the image is refused
    through the device's flag"""
    from pointnerf_amd import ops
    f32 = dict(dtype=torch.float32, device=dev)
    canv = [torch.full((h, w), 7.0, **f32) for _ in range(3)]
    vals = [torch.tensor([1.0, 2.0, 3.0], **f32) for _ in range(3)]
    mask = torch.tensor([1, 0, 1], dtype=torch.int8, device=dev)
    ops.geometry_canvas(torch.tensor([[0, 0], [5, 1], [w - 1, h - 1]], device=dev), mask, *vals, canv)
    for cv in canv:
        c = cv.cpu()
        assert c[0, 0] == 1.0 and c[1, 5] == 0.0 and c[h - 1, w - 1] == 3.0 and int((c == 7.0).sum()) == h * w - 3
    for bad in ([w, 0], [0, h], [-1, 0], [0, -1]):
        with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
            ops.geometry_canvas(torch.tensor([[1, 1], bad, [2, 2]], device=dev), None, *vals, canv)
    c = canv[0].cpu()
    assert c[1, 1] == 1.0 and c[2, 2] == 3.0 and int((c == 7.0).sum()) == h * w - 5             # the in-range rays of a refused call were written

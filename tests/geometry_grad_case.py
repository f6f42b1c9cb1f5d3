"""Depth and mask supervision: the GEOM instance of k_raymarch_backward behind pnerf_raymarch_backward_geom /
pnerf_render_backward_geom, the fused loss pass (ops.GeometryLossRays) and the ``geometry_grad`` switch of the model, shared by the
host-emulator twin tests/test_geometry_grad_emu.py and by tests/test_gpu_geometry_grad.py.

1. The kernel alone.  The cases, inputs and bars are tests/raymarch_case.py's, unchanged; added are a per-slot depth ``z`` (increasing along
the ray, roughly 2 .. 6) and per-ray gradients ``grad_geom`` = (g_ds, g_acc, g_T) with both signs, seeded.  The yardstick is the float64
autograd of  g . colour + g_ds sum_s bw_s z_s + g_acc sum_s bw_s + g_T T_end  (``march_geom`` below, next to raymarch_case.march), the
comparison the fp32 autograd of the same formula; per ray E = max_s |d - d64| / max_s |d64| of d sigma, the kernel's median / p95 / max at
most BACKWARD_MARGIN x the fp32 autograd's (opaque: the rays where the fp32 autograd is within OPAQUE_ORACLE_E, there E <= OPAQUE_HIP_E, at
most OPAQUE_LEFT_OUT of the rays left out).  Two variants: "geom" (zero colour gradient) and "both".

2. The loss pass against a float64 numpy statement, with derived bounds (``check_loss_pass``).

3. Through the model on the device against oracle/pyref.py (``model_step`` / ``oracle_step``): depth_sum, acc and T_end restated from the
oracle's own blend weights, validity and sample positions, under autograd."""
import ctypes

import numpy as np
import torch

import raymarch_case as RC

VARIANTS = ("geom", "both")
# seeds of z / grad_geom for which the fp32 autograd ALONE leaves out at most OPAQUE_LEFT_OUT of the rays of every opaque case (checked on the
# CPU when the feature was specified; GeomReference.check_conditions asserts it)
GEOM_SEED = 5


def march_geom(dist, valid, feats, z, bg):
    """raymarch_case.march plus the three geometry outputs, in the dtype of ``feats``: depth_sum = sum_s bw_s z_s over the valid slots,
    acc = sum_s bw_s, T_end"""
    out = RC.march(dist, valid, feats, bg)
    bw = out["blend_weight"]
    zz = torch.where(valid, z.to(feats.dtype), torch.zeros((), dtype=feats.dtype))
    return dict(ray_color=out["ray_color"], depth_sum=(bw * zz).sum(dim=-1), acc=bw.sum(dim=-1), T_end=out["background_transmission"])


def geom_inputs(base):
    """(z [R,SR] f32, grad_geom [R,3] f32) for a raymarch_case.Reference: z rises along the ray from about 2 to about 6; grad_geom is normal,
    both signs, and zero on the rays built with a zero colour gradient (they stay dead)"""
    gen = torch.Generator().manual_seed(7000 * GEOM_SEED + base.SR)
    step = 0.05 + torch.rand(RC.R, base.SR, generator=gen)
    z = 2.0 + 4.0 * torch.cumsum(step, dim=1) / step.sum(dim=1, keepdim=True)
    gg = torch.randn(RC.R, 3, generator=gen)
    for r in base.rows["zero_grad"]:
        gg[r] = 0.0
    return z.float().contiguous(), gg.float().contiguous()


def _sigma_error(d, d64):
    d = d.double()
    err = (d[..., 0] - d64[..., 0]).abs().max(dim=1).values
    top = d64[..., 0].abs().max(dim=1).values
    return torch.where(top > 0, err / top, torch.full_like(err, float("nan")))


class GeomReference:
    """One (case, variant): raymarch_case's inputs plus z and grad_geom, the float64 gradient, the fp32 autograd's and its per-ray error"""

    def __init__(self, case, variant):
        torch.set_num_threads(8)
        self.base = RC.reference(case)
        self.case, self.variant, self.kind, self.SR = case, variant, self.base.kind, self.base.SR
        b = self.base
        self.z, self.gg = geom_inputs(b)
        self.g = b.g if variant == "both" else torch.zeros_like(b.g)
        self.d64 = self._grad(torch.float64)
        self.d32 = self._grad(torch.float32)
        self.E32 = _sigma_error(self.d32, self.d64)

    def _grad(self, dt):
        b = self.base
        f = b.feats.to(dt).requires_grad_(True)
        o = march_geom(b.dist.to(dt), b.valid, f, self.z.to(dt), b.bg)
        gg = self.gg.to(dt)
        scalar = (o["ray_color"] * self.g.to(dt)).sum() + (o["depth_sum"] * gg[:, 0]).sum() + (o["acc"] * gg[:, 1]).sum() + (o["T_end"] * gg[:, 2]).sum()
        d, = torch.autograd.grad(scalar, f)
        return d.detach()

    def counted(self):
        e = self.E32
        if self.kind == "opaque":
            return ~torch.isnan(e) & (e <= RC.OPAQUE_ORACLE_E)
        return ~torch.isnan(e)

    def check_conditions(self):
        """on the fp32 autograd alone: d sigma vanishes exactly on the dead rays, and an opaque case leaves out at most OPAQUE_LEFT_OUT"""
        b = self.base
        dead = ~(b.valid & (b.dist > 0)).any(dim=1) | ((self.g == 0).all(dim=1) & (self.gg == 0).all(dim=1))
        assert torch.equal(torch.isnan(self.E32), dead), (self.case, self.variant)
        n_out = int((~dead).sum()) - int(self.counted().sum())
        assert int(self.counted().sum()) >= RC.R // 2 and n_out <= RC.OPAQUE_LEFT_OUT * RC.R, (self.case, self.variant, "rays left out", n_out, RC.R)
        assert float(self.z.min()) >= 2.0 and float(self.z.max()) <= 6.0 + 1e-5 and bool((self.z[:, 1:] > self.z[:, :-1]).all())
        assert bool((self.gg > 0).any()) and bool((self.gg < 0).any())


_refs = {}


def reference(case, variant):
    key = (case, variant)
    if key not in _refs:
        _refs[key] = GeomReference(case, variant)
        _refs[key].check_conditions()
    return _refs[key]


# ---- the two entry points -------------------------------------------------------------------------------------------------------------------

def _c(dev):
    from pointnerf_amd import _lib as L, ops
    return L.lib(), ops._ptr, ops._stream


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _bg3(bg):
    return None if bg is None else (ctypes.c_float * 3)(*bg.tolist())


def hip_backward_geom(ref, dev, g=None, gg=None, z=None, rows=None):
    """pnerf_raymarch_backward_geom on the case (optionally other gradients / depths, or a slice of the rays) -> d feats [R,SR,4] on the CPU"""
    lib, ptr, stream = _c(dev)
    b = ref.base
    sel = slice(None) if rows is None else rows
    t = lambda a: a[sel].contiguous().to(dev)
    dist, valid, feats = t(b.dist), t(b.valid.to(torch.uint8)), t(b.feats)
    zz, g_, gg_ = t(ref.z if z is None else z), t(ref.g if g is None else g), t(ref.gg if gg is None else gg)
    n = dist.shape[0]
    out = torch.full((n, b.SR, 4), float("nan"), device=dev)
    rc = lib.pnerf_raymarch_backward_geom(ptr(dist), ptr(valid), ptr(feats), ptr(zz), _bg3(b.bg), n, b.SR, ptr(g_), ptr(gg_), ptr(out), stream())
    assert rc == 0, rc
    _sync(dev)
    return out.cpu()


def hip_backward_plain(ref, dev, g=None):
    """pnerf_raymarch_backward (the existing entry) on the same inputs"""
    lib, ptr, stream = _c(dev)
    b = ref.base
    t = lambda a: a.contiguous().to(dev)
    dist, valid, feats, g_ = t(b.dist), t(b.valid.to(torch.uint8)), t(b.feats), t(ref.g if g is None else g)
    out = torch.full((RC.R, b.SR, 4), float("nan"), device=dev)
    assert lib.pnerf_raymarch_backward(ptr(dist), ptr(valid), ptr(feats), _bg3(b.bg), RC.R, b.SR, ptr(g_), ptr(out), stream()) == 0
    _sync(dev)
    return out.cpu()


def check_backward(ref, grad, margin=RC.BACKWARD_MARGIN):
    """the per-ray figures of d sigma, printed before anything is asserted (raymarch_case.check_backward's table and bars)"""
    assert bool(torch.isfinite(grad).all()), (ref.case, ref.variant)
    E = _sigma_error(grad, ref.d64)
    m = ref.counted()
    qh, qo = RC.quantiles(E[m]), RC.quantiles(ref.E32[m])
    tag = "%s/%s" % (RC.case_id(ref.case), ref.variant)
    bad = []
    for q in ("median", "p95", "max"):
        asserted = ref.kind != "opaque" or q == "median"
        over = asserted and not qh[q] <= margin * qo[q]
        print("%-30s d sigma  E over %3d rays  %-6s hip %.2e   fp32 autograd %.2e   ratio %5.2f%s%s" % (
            tag, int(m.sum()), q, qh[q], qo[q], qh[q] / qo[q] if qo[q] > 0 else float("inf"),
            "" if asserted else "   (not asserted)", "   <-- beyond %.1f x the autograd" % margin if over else ""))
        if over:
            bad.append((q, qh[q], qo[q]))
    if ref.kind == "opaque" and not qh["max"] <= RC.OPAQUE_HIP_E:
        print("%-30s d sigma  E max %.2e on the counted rays   <-- beyond %.0e" % (tag, qh["max"], RC.OPAQUE_HIP_E))
        bad.append(("max on counted rays", qh["max"], RC.OPAQUE_HIP_E))
    assert not bad, (ref.case, ref.variant, bad)


def check_rgb_unchanged_and_invalid_slots(ref, grad, dev):
    """d rgb is pnerf_raymarch_backward's for the same colour gradient, bit for bit; no gradient on an invalid slot"""
    plain = hip_backward_plain(ref, dev)
    assert torch.equal(grad[..., 1:], plain[..., 1:]), (ref.case, ref.variant, "d rgb changed")
    inv = ~ref.base.valid
    assert torch.equal(grad[inv], torch.zeros(int(inv.sum()), 4)), "a gradient on an invalid slot"
    for r in ref.base.rows["empty"] + ref.base.rows["zero_grad"]:
        assert torch.equal(grad[r], torch.zeros(ref.SR, 4)), (ref.case, r)


def check_zero_geom_is_plain(ref, dev):
    """grad_geom = 0: the values of pnerf_raymarch_backward (c + 0 z + 0 and S_bg + 0 are exact in double; torch.equal: a zero's sign aside)"""
    b = ref.base
    got = hip_backward_geom(ref, dev, g=b.g, gg=torch.zeros_like(ref.gg))
    plain = hip_backward_plain(ref, dev, g=b.g)
    assert float(plain.abs().max()) > 0
    assert torch.equal(got, plain), (ref.case, "zero grad_geom differs from pnerf_raymarch_backward")


def check_scaling(ref, dev):
    """grad_geom and the colour gradient x 2^k: d sigma x 2^k exactly.  On the random rays of a thin case (raymarch_case.check_scaling)"""
    assert ref.kind == "thin"
    b = ref.base
    rows = slice(0, min(sum(b.rows.values(), [])))
    base = hip_backward_geom(ref, dev, rows=rows)
    assert float(base[..., 0].abs().max()) > 0
    for p in (-30, 20):
        gs = hip_backward_geom(ref, dev, g=ref.g * 2.0 ** p, gg=ref.gg * 2.0 ** p, rows=rows)
        assert torch.equal(gs * 2.0 ** -p, base), (ref.case, ref.variant, "x 2^%d" % p)


def check_ray_alone(ref, grad, dev, r):
    g1 = hip_backward_geom(ref, dev, rows=slice(r, r + 1))
    assert torch.equal(g1[0], grad[r]), (ref.case, ref.variant, r)


def check_poisoned_z(ref, grad, dev):
    """NaN in z on every invalid slot: nothing changes"""
    z = ref.z.clone()
    z[~ref.base.valid] = float("nan")
    assert bool(torch.isnan(z).any())
    assert torch.equal(hip_backward_geom(ref, dev, z=z), grad), (ref.case, ref.variant, "z of an invalid slot reached the gradient")


def check_guarded_memory(ref, grad, dev, pad=256):
    """every array carved out of a larger buffer whose surroundings hold NaN (valid flags: 1): the same bits, nothing written outside"""
    lib, ptr, stream = _c(dev)
    b = ref.base
    nan = float("nan")
    ins = {}
    for name, t, dt, fill in (("dist", b.dist, torch.float32, nan), ("valid", b.valid.to(torch.uint8), torch.uint8, 1), ("feats", b.feats, torch.float32, nan),
                              ("z", ref.z, torch.float32, nan), ("g", ref.g, torch.float32, nan), ("gg", ref.gg, torch.float32, nan)):
        ins[name] = RC._carve(dev, t.numel(), dt, pad, fill)
        ins[name][1].copy_(t.flatten().to(dev))
    big, view = RC._carve(dev, 4 * RC.R * b.SR, torch.float32, pad, nan)
    p = lambda k: ptr(ins[k][1])
    assert lib.pnerf_raymarch_backward_geom(p("dist"), p("valid"), p("feats"), p("z"), _bg3(b.bg), RC.R, b.SR, p("g"), p("gg"), ptr(view), stream()) == 0
    _sync(dev)
    assert torch.equal(view.cpu(), grad.flatten()), (ref.case, "depends on the memory around the arrays")
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all()), (ref.case, "written outside the array")


def check_return_codes(dev):
    """pnerf_raymarch_backward_geom: pnerf_raymarch_backward's checks -- PNERF_E_INVAL for SR <= 0, R < 0 and each null pointer but bg3_host,
    PNERF_E_UNSUP for SR > 4096, 0 and nothing written for R == 0"""
    lib, ptr, stream = _c(dev)
    INVAL, UNSUP = -1, -4
    Rn, SR, nan = 3, 5, float("nan")
    dist = torch.full((Rn, SR), 0.01, device=dev)
    valid = torch.ones(Rn, SR, dtype=torch.uint8, device=dev)
    feats = torch.ones(Rn, SR, 4, device=dev)
    z = torch.full((Rn, SR), 3.0, device=dev)
    g, gg = torch.ones(Rn, 3, device=dev), torch.ones(Rn, 3, device=dev)
    gf = torch.full((Rn, SR, 4), nan, device=dev)
    bg3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def call(R_=Rn, SR_=SR, bg=bg3, null=None):
        a = [ptr(dist), ptr(valid), ptr(feats), ptr(z), ptr(g), ptr(gg), ptr(gf)]
        if null is not None:
            a[null] = ptr(None)
        return lib.pnerf_raymarch_backward_geom(a[0], a[1], a[2], a[3], bg, R_, SR_, a[4], a[5], a[6], stream())

    assert call(SR_=0) == INVAL and call(SR_=-1) == INVAL and call(R_=-1) == INVAL
    for i in range(7):
        assert call(null=i) == INVAL, ("null pointer", i)
    assert call(R_=0) == 0 and call(SR_=4097) == UNSUP
    _sync(dev)
    assert bool(torch.isnan(gf).all()), "a refused or empty call wrote to its output"
    assert call(bg=None) == 0
    _sync(dev)
    assert bool(torch.isfinite(gf).all())


def check_render_backward_geom_return_codes(dev):
    """pnerf_render_backward_geom validates like pnerf_render_backward: null records and a null gradient are PNERF_E_INVAL before anything
    is read"""
    from pointnerf_amd import _lib as L
    lib, ptr, stream = _c(dev)
    cam, pts, st, pg = L.Camera(), L.Points(), L.Step(), L.PointGrads()
    null = ptr(None)
    args = lambda c, p, s: (c, p, s, null, null, null, null, null, null, ctypes.byref(pg), null, 0, stream())
    assert lib.pnerf_render_backward_geom(*args(None, ctypes.byref(pts), ctypes.byref(st))) == -1
    assert lib.pnerf_render_backward_geom(*args(ctypes.byref(cam), None, ctypes.byref(st))) == -1
    assert lib.pnerf_render_backward_geom(*args(ctypes.byref(cam), ctypes.byref(pts), None)) == -1
    st.R, st.SR, st.K = 4, 8, 4
    assert lib.pnerf_render_backward_geom(*args(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st))) == lib.pnerf_render_backward(
        ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), null, null, null, null, null, ctypes.byref(pg), null, 0, stream()) != 0


# ---- 2. the loss pass -------------------------------------------------------------------------------------------------------------------------
LOSS_R = 253
MASKS = ("binary", "fractional")
# Rounded fp32 operations per term, read from PnGeomRay / the two kernels of csrc/loss.hip:
#   depth term: acc + 1e-6, 1 / ., depth_sum * inv, d - gt, m * ., the square                      = 6
#   bg term:    1 - m, T - 1, w * ., the square                                                    = 4
#   g_ds:       the 5 of m (d - gt), then m * ., 2 gscale (exact) * ., * inv                       = 8
#   g_acc:      g_ds, then * d (d itself carries 3 more)                                           = 12
#   g_T:        the 3 of w (T - 1), then w * ., 2 gscale * .                                       = 5
N_TERM, N_GRAD = 6, 12


def loss_inputs(mask_kind, seed=3):
    """R = 253 rays, about a fifth of them misses (their depth_sum / acc / T hold NaN: a miss's rows are not read); acc from thin to opaque"""
    rng = np.random.default_rng(seed)
    R = LOSS_R
    hit = (rng.random(R) > 0.2).astype(np.int32)
    acc = np.where(rng.random(R) < 0.3, rng.uniform(1e-3, 0.05, R), rng.uniform(0.05, 1.0, R)).astype(np.float32)
    depth = rng.uniform(2.0, 6.0, R)
    depth_sum = (depth * acc).astype(np.float32)
    T = (1.0 - acc * rng.uniform(0.8, 1.0, R)).astype(np.float32)
    gt = rng.uniform(2.0, 6.0, R).astype(np.float32)
    m = (rng.random(R) < 0.6).astype(np.float32)
    if mask_kind == "fractional":
        frac = rng.random(R) < 0.4
        m = np.where(frac, rng.random(R), m).astype(np.float32)
    for a in (depth_sum, acc, T):
        a[hit == 0] = np.nan
    return dict(depth_sum=depth_sum, acc=acc, T=T, hit=hit, gt=gt, m=m)


def loss_restatement(x, gs=(1.0, 1.0)):
    """float64 numpy statement of DESIGN.md 4.10's loss pass on the fp32 inputs -> (N_depth, N_bg, grad_geom [R,3], |grad| with |d - gt| -> |d| + |gt|)"""
    hit = x["hit"] > 0
    f = lambda a: np.where(hit, np.nan_to_num(a.astype(np.float64)), 0.0)
    ds, acc, m, gt = f(x["depth_sum"]), f(x["acc"]), x["m"].astype(np.float64), x["gt"].astype(np.float64)
    T = np.where(hit, np.nan_to_num(x["T"].astype(np.float64)), 1.0)
    inv = 1.0 / (acc + np.float64(np.float32(1e-6)))
    d = np.where(hit, ds * inv, 0.0)
    nd, nb = (m * m * (d - gt) ** 2).sum(), ((1 - m) ** 2 * (T - 1) ** 2).sum()
    g_ds = np.where(hit, gs[0] * 2 * m * m * (d - gt) * inv, 0.0)
    g_T = np.where(hit, gs[1] * 2 * (1 - m) ** 2 * (T - 1), 0.0)
    grad = np.stack([g_ds, -g_ds * d, g_T], 1)
    big_ds = np.where(hit, abs(gs[0]) * 2 * m * m * (np.abs(d) + np.abs(gt)) * inv, 0.0)
    big = np.stack([big_ds, big_ds * np.abs(d), np.abs(g_T)], 1)
    return nd, nb, grad, big


def check_loss_pass(mask_kind, dev):
    """numerators: sums of non-negative terms, each term within n 2^-24 relative and the sum of R of them within R 2^-24 more: relative error at
    most (R + N_TERM) 2^-24.  Gradients: per ray within N_GRAD 2^-24 of the value with |d - gt| replaced by |d| + |gt| (the subtraction is where
    the roundings of d are amplified).  Misses: zeros, and their (NaN) rows are not read."""
    from pointnerf_amd import ops
    x = loss_inputs(mask_kind)
    if mask_kind == "binary":
        assert set(np.unique(x["m"])) == {0.0, 1.0}
    else:
        assert ((x["m"] > 0) & (x["m"] < 1)).sum() > 50 and (x["m"] == 0).any() and (x["m"] == 1).any()
    assert 20 < int((x["hit"] == 0).sum()) < LOSS_R // 2
    gs = (0.75, -1.5)
    nd, nb, grad, big = loss_restatement(x, gs)
    t = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    leaves = [t[k].clone().requires_grad_(True) for k in ("depth_sum", "acc", "T")]
    got_d, got_b = ops.geometry_loss_sums_rays(leaves[0], leaves[1], leaves[2], t["hit"], t["gt"], t["m"])
    (gs[0] * got_d + gs[1] * got_b).backward()
    _sync(dev)
    eps = 2.0 ** -24
    e_d, e_b = abs(float(got_d.detach()) - nd) / nd, abs(float(got_b.detach()) - nb) / nb
    print("loss pass (%s): N_depth %.6g rel err %.2e, N_bg %.6g rel err %.2e, bound %.2e" % (mask_kind, nd, e_d, nb, e_b, (LOSS_R + N_TERM) * eps))
    assert e_d <= (LOSS_R + N_TERM) * eps and e_b <= (LOSS_R + N_TERM) * eps, (e_d, e_b)
    g = torch.stack([l.grad for l in leaves], 1).cpu().double().numpy()
    hit = x["hit"] > 0
    assert np.array_equal(g[~hit], np.zeros((int((~hit).sum()), 3))), "a gradient on a ray that missed"
    err = np.abs(g - grad)
    worst = float((err[hit] / np.maximum(big[hit], 1e-300)).max())
    print("loss pass (%s): gradients, worst error / (N_GRAD 2^-24 x the un-cancelled value) = %.3f" % (mask_kind, worst / (N_GRAD * eps)))
    assert (err <= N_GRAD * eps * big).all(), worst


# ---- 3. through the model, on the device --------------------------------------------------------------------------------------------------
W_DEPTH, W_BG = 0.05, 0.5
MODEL_CASE = "small_k4"


def supervision(R, seed=11):
    """gt_depth [1,R,1] around the scene's depths and gt_mask [1,R,1]: zeros, ones and fractional values"""
    gen = torch.Generator().manual_seed(seed)
    gt_depth = 3.0 + 2.0 * torch.rand(1, R, 1, generator=gen)
    m = (torch.rand(1, R, 1, generator=gen) < 0.6).float()
    frac = torch.rand(1, R, 1, generator=gen) < 0.3
    return gt_depth, torch.where(frac, torch.rand(1, R, 1, generator=gen), m)


def oracle_geometry_losses(out, gt_depth, gt_mask):
    """depth_sum, acc and T_end restated from an oracle render's own blend weights, validity and sample positions (the hit rays), filled to
    all R rays as fill_invalid does (depth 0, T 1 on a miss), and the two l2 losses of base_rendering_model.py:610-626 on them"""
    mask = out["ray_mask"][0] > 0
    R = mask.numel()
    bw = out["blend_weight"][0, ..., 0]
    valid = out["ray_valid"][0]
    z = out["query"]["sample_loc"][0, ..., 2].to(bw.dtype)
    depth_sum = (bw * torch.where(valid, z, torch.zeros((), dtype=bw.dtype))).sum(-1)
    acc = bw.sum(-1)
    T = out["coarse_is_background"][0, :, 0]
    d_full = torch.zeros(R, dtype=bw.dtype).index_put((mask.nonzero()[:, 0],), depth_sum / (acc + 1e-6))
    T_full = torch.ones(R, dtype=bw.dtype).index_put((mask.nonzero()[:, 0],), T)
    m, gt = gt_mask.reshape(-1).to(bw.dtype), gt_depth.reshape(-1).to(bw.dtype)
    l_depth = torch.nn.functional.mse_loss(d_full * m, gt * m)
    l_bg = torch.nn.functional.mse_loss(T_full * (1 - m), 1 - m)
    return dict(depth_sum=depth_sum, acc=acc, T=T, depth=depth_sum / (acc + 1e-6), l_depth=l_depth, l_bg=l_bg)


def build_trainable(case, dev, geometry_grad=True):
    from pointnerf_amd.neural_points import NeuralPoints
    from pointnerf_amd.neural_points_volumetric_model import NeuralPointsRayMarching
    from pointnerf_amd.point_aggregators import PointAggregator
    opt, xyz, attrs, inp, mlp = case
    agg = PointAggregator(opt).to(dev)
    agg.load_state_dict(mlp)
    agg.flatten_()
    npnt = NeuralPoints(32, xyz.shape[0], opt, torch.device(dev))
    a = {k: v.to(dev) for k, v in attrs.items()}
    npnt.set_points(xyz.to(dev), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"], parameter=True)
    model = NeuralPointsRayMarching(aggregator=agg, neural_points=npnt, opt=opt)
    model.geometry_grad = geometry_grad
    d = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    return model, agg, npnt, d


def model_step(case, dev, gt_depth, gt_mask):
    """one forward + backward of  W_DEPTH L_depth + W_BG L_bg + the colour / zero-one loss  through the fused node -> (values, gradients)"""
    from oracle import pyref
    from pointnerf_amd import losses
    model, agg, npnt, d = build_trainable(case, dev)
    out = model(**d)
    R = out["ray_mask"].shape[1]
    nd, count = losses.depth(out, gt_depth.to(dev), gt_mask.to(dev))
    nb, _ = losses.background(out, gt_mask.to(dev))
    assert count == R
    loss = W_DEPTH * nd / R + W_BG * nb / R + pyref.training_loss(case[0], out, {"gt_image": d["gt_image"]})
    loss.backward()
    dg = out["_dense_geometry"]
    hit = (dg[3] > 0).cpu()
    vals = dict(depth_sum=dg[0].detach().cpu()[hit], acc=dg[1].detach().cpu()[hit], T=dg[2].detach().cpu()[hit], l_depth=float(nd) / R, l_bg=float(nb) / R)
    g = {n: p.grad.detach().cpu().clone() for n, p in agg.named_parameters()}
    g.update({n: getattr(npnt, n).grad.detach().cpu().clone() for n in ("points_embeding", "points_conf", "points_dir", "points_color")})
    return vals, g


def oracle_step(case, gt_depth, gt_mask):
    from oracle import pyref
    opt, xyz, attrs, inp, mlp = case
    torch.set_num_threads(8)
    om = {k: v.clone().requires_grad_(True) for k, v in mlp.items()}
    op = dict(xyz=xyz, **{k: v.clone().requires_grad_(True) for k, v in attrs.items()})
    out = pyref.render(opt, op, om, inp, nthreads=8)
    geo = oracle_geometry_losses(out, gt_depth, gt_mask)
    (W_DEPTH * geo["l_depth"] + W_BG * geo["l_bg"] + pyref.training_loss(opt, out, inp)).backward()
    g = {k: v.grad for k, v in om.items()}
    g.update({k: op[k].grad for k in attrs})
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in geo.items()}, g

"""The ray march ALONE (k_raymarch_forward / k_raymarch_backward behind pointnerf_amd.diff_ray_marching.ray_march) against float64, per slot
and per ray (test infrastructure, shared by tests/test_gpu_raymarch.py and the host-emulator twin tests/test_raymarch_emu.py, as range_case.py
serves the gradient-range tests).

Inputs are BUILT for the ray march instead of coming out of a render of a thin random scene: R = 253 rays (no multiple of the 4 rays of a
workgroup) of SR in {1, 63, 64, 65, 130, 160} slots (one chunk short of, at and past the 64-slot seam; two seams; a ragged third chunk),
sigma = softplus(3 randn) x scale with scale 1 ("thin": rays keep about half their transmittance), 30 ("mixed") and 300 ("opaque": the visible
part of a ray is a hard surface), and a few hand-built rays in every case: no valid slot, one valid slot, a thin front with one opaque slot
at or next to a chunk seam and matter behind it, delta = 0 on valid slots, a zero colour gradient.

The float64 yardstick and the fp32 oracle are `march` below, the formula of diff_ray_marching.py:508-554 in torch (pinned to oracle/pyref.py's
ray_march by the tests), in float64 and in float32 with autograd.  Gradients are compared PER RAY:

    E(ray) = max_s |d - d64| / max_s |d64|        for d sigma and, over slots and channels, for d rgb

for the HIP path and for the fp32 oracle; what is asserted are the ratios of the kernel's quantiles of E to the oracle's (BACKWARD_MARGIN): a
ray that is dim because something opaque sits in front of it has to be as accurate, relative to its OWN gradient, as fp32 arithmetic allows."""
import ctypes

import numpy as np
import torch

R = 253
SRS = (1, 63, 64, 65, 130, 160)
SCALE = {"thin": 1.0, "mixed": 30.0, "opaque": 300.0}
BGS = {"thin": ("white",), "mixed": ("none", "tint"), "opaque": ("white",)}
BG = {"white": (1.0, 1.0, 1.0), "tint": (0.2, 0.7, 1.0), "none": None}
# seeds for which the fp32 ORACLE alone meets Reference.check_conditions with room (opaque: 25 % of the rays left out at the most)
SEED = {"thin": 0, "mixed": 1, "opaque": 2}

FORWARD_BAR = 1.2e-6            # the project's forward bar (README, Parity): max |hip - f64| per element of every forward output
BACKWARD_MARGIN = 2.0           # kernel quantile of E <= margin x the oracle's same quantile (the kernel adds in a wave-tree order, the oracle in sequence)
OPAQUE_ORACLE_E = 1e-5          # opaque: a ray counts where the fp32 oracle's own E is at most this ...
OPAQUE_HIP_E = 2e-5             # ... and there the kernel's E is at most this
OPAQUE_LEFT_OUT = 0.25          # ... and the rays left out are at most this share of R (a condition on the case)
SURFACE_OD = (3.0, 8.0, 14.0, 20.0, 30.0, 100.0)
SURFACE_SLOT = (5, 63, 64)
FORWARD_KEYS = ("ray_color", "opacity", "acc_transmission", "blend_weight", "background_transmission")

CASES = [(kind, SR, bg) for kind in ("thin", "mixed", "opaque") for SR in SRS for bg in BGS[kind]]


def case_id(c):
    return "%s-SR%d-bg_%s" % c


def march(dist, valid, feats, bg):
    """diff_ray_marching.py:508-554 with radiance_render / alpha_blend, in the dtype of `feats`: dist, valid [R,SR], feats [R,SR,4], bg None or
    [3].  Imports nothing of the code under test."""
    dt = feats.dtype
    sigma = feats[..., 0] * valid.to(dt)
    op = 1 - torch.exp(-sigma * dist.to(dt))
    u = 1 - op + 1e-10
    acc = torch.cumprod(u, dim=-1)
    T_end = acc[:, -1]
    T = torch.cat([torch.ones_like(acc[:, :1]), acc[:, :-1]], dim=-1)
    bw = op * T
    color = (bw[..., None] * feats[..., 1:4]).sum(dim=-2)
    if bg is not None:
        color = color + bg.to(dt)[None, :] * T_end[:, None]
    return dict(ray_color=color, opacity=op, acc_transmission=T, blend_weight=bw, background_transmission=T_end)


def build_inputs(kind, SR, seed):
    """(dist [R,SR] f32, valid [R,SR] bool, feats [R,SR,4] f32, g [R,3] f32, rows: name -> list of hand-built ray numbers), all on the CPU"""
    gen = torch.Generator().manual_seed(1000 * seed + SR)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    valid = rnd(R, SR) > 0.3
    dist = (0.002 + 0.01 * rnd(R, SR)) * valid
    sigma = torch.nn.functional.softplus(3 * torch.randn(R, SR, generator=gen)) * SCALE[kind]
    feats = torch.cat([sigma[..., None], rnd(R, SR, 3)], dim=-1)
    g = torch.randn(R, 3, generator=gen)
    rows = {"empty": [], "single": [], "surface": [], "zero_dist": [], "zero_grad": []}
    nxt = [R - 1]

    def take(name):
        r = nxt[0]
        nxt[0] -= 1
        rows[name].append(r)
        return r

    r = take("empty")
    valid[r] = False
    dist[r] = 0.0
    for s in sorted({0, 63, 64, SR - 1}):
        if s < SR:
            r = take("single")
            valid[r] = False
            valid[r, s] = True
            dist[r] = dist[r] * valid[r]
            if dist[r, s] == 0:
                dist[r, s] = 0.007
    for slot in SURFACE_SLOT:
        if slot >= SR:
            continue
        for od in SURFACE_OD:
            r = take("surface")
            valid[r] = True
            dist[r] = 0.01
            sd = 2.0 * rnd(SR)
            sd[:slot] = 0.02 * rnd(slot)
            sd[slot] = od
            feats[r, :, 0] = sd / 0.01
    r = take("zero_dist")                           # delta = 0 on every valid slot: the ray composites nothing
    valid[r] = True
    dist[r] = 0.0
    r = take("zero_dist")                           # delta = 0 on every other valid slot
    dist[r, 0::2] = 0.0
    r = take("zero_grad")
    g[r] = 0.0
    return dist.contiguous(), valid.contiguous(), feats.contiguous(), g.contiguous(), rows


def per_ray_error(d, d64):
    """(E_sigma [R], E_rgb [R]) of a gradient [R,SR,4] against the float64 one; nan on a ray whose float64 gradient is identically 0"""
    d = d.double()
    out = []
    for lo, hi in ((0, 1), (1, 4)):
        err = (d[..., lo:hi] - d64[..., lo:hi]).abs().flatten(1).max(dim=1).values
        top = d64[..., lo:hi].abs().flatten(1).max(dim=1).values
        out.append(torch.where(top > 0, err / top, torch.full_like(err, float("nan"))))
    return out


class Reference:
    """One case: its inputs, the float64 outputs and gradients, the fp32 oracle's, and the oracle's own per-ray errors."""

    def __init__(self, case):
        torch.set_num_threads(8)
        self.case = case
        self.kind, self.SR, self.bg_name = case
        self.dist, self.valid, self.feats, self.g, self.rows = build_inputs(self.kind, self.SR, SEED[self.kind])
        self.bg = None if BG[self.bg_name] is None else torch.tensor(BG[self.bg_name])
        f64 = self.feats.double().requires_grad_(True)
        self.out64 = march(self.dist.double(), self.valid, f64, self.bg)
        self.d64, = torch.autograd.grad((self.out64["ray_color"] * self.g.double()).sum(), f64)
        self.out64 = {k: v.detach() for k, v in self.out64.items()}
        f32 = self.feats.clone().requires_grad_(True)
        self.out32 = march(self.dist, self.valid, f32, self.bg)
        self.d32, = torch.autograd.grad((self.out32["ray_color"] * self.g).sum(), f32)
        self.out32 = {k: v.detach() for k, v in self.out32.items()}
        self.E32 = per_ray_error(self.d32, self.d64)

    def counted(self, i):
        """the rays whose E (0: d sigma, 1: d rgb) enters the statistics"""
        e = self.E32[i]
        if self.kind == "opaque":
            return ~torch.isnan(e) & (e <= OPAQUE_ORACLE_E)
        return ~torch.isnan(e)

    def check_conditions(self):
        """conditions on the CASE, not measurements, asserted on the oracle alone: the hand-built rays are there, the float64 gradient
        vanishes on the rays built for that and on no other, the oracle's forward is inside the bar, and an opaque case leaves out at most
        OPAQUE_LEFT_OUT of its rays"""
        assert len(self.rows["empty"]) == 1 and len(self.rows["single"]) >= 1 and len(self.rows["zero_dist"]) == 2
        assert len(self.rows["surface"]) == len(SURFACE_OD) * sum(s < self.SR for s in SURFACE_SLOT)
        dead = ~(self.valid & (self.dist > 0)).any(dim=1) | (self.g == 0).all(dim=1)       # composites nothing, or is not looked at
        for r in self.rows["empty"] + self.rows["zero_grad"] + self.rows["zero_dist"][:1]:
            assert bool(dead[r]), (self.case, r)
        for i in (0, 1):
            assert torch.equal(torch.isnan(self.E32[i]), dead), (self.case, i, "the float64 gradient vanishes exactly on the dead rays")
            n_out = int((~dead).sum()) - int(self.counted(i).sum())
            assert int(self.counted(i).sum()) >= R // 2 and n_out <= OPAQUE_LEFT_OUT * R, (self.case, "rays left out", n_out, R)
        for k in FORWARD_KEYS:
            assert float((self.out32[k].double() - self.out64[k]).abs().max()) <= FORWARD_BAR, (self.case, k)


def check_pinned_to_pyref(pyref):
    """`march` IS oracle/pyref.py's ray_march (the reference formula the whole suite compares renders with): same bits in fp32 and float64,
    outputs and gradient, on a mixed case with a background and on one without"""
    for case in (("mixed", 65, "tint"), ("mixed", 130, "none")):
        ref = Reference(case)
        for dt in (torch.float32, torch.float64):
            f = [ref.feats.to(dt).requires_grad_(True) for _ in range(2)]
            mine = march(ref.dist.to(dt), ref.valid, f[0], ref.bg)
            color, _, op, acc, bw, bg_t = pyref.ray_march(ref.dist.to(dt)[None], ref.valid[None], f[1][None], None if ref.bg is None else ref.bg[None])
            theirs = dict(ray_color=color[0], opacity=op[0], acc_transmission=acc[0], blend_weight=bw[0, ..., 0], background_transmission=bg_t[0, :, 0])
            for k in FORWARD_KEYS:
                assert torch.equal(mine[k], theirs[k]), (case, dt, k)
            ga, = torch.autograd.grad((mine["ray_color"] * ref.g.to(dt)).sum(), f[0])
            gb, = torch.autograd.grad((theirs["ray_color"] * ref.g.to(dt)).sum(), f[1])
            assert torch.equal(ga, gb), (case, dt)


_refs = {}


def reference(case):
    if case not in _refs:
        _refs[case] = Reference(case)
        _refs[case].check_conditions()
    return _refs[case]


# ---- the HIP path ----------------------------------------------------------------------------------------------------------------------

def hip_march(dist, valid, feats, g, bg, dev):
    """ray_march() forward and backward on CPU inputs [R,SR] / [R,3]; returns (forward outputs, d feats [R,SR,4]) as float32 CPU tensors"""
    from pointnerf_amd.diff_ray_marching import ray_march
    from pointnerf_amd.diff_render_func import radiance_render, alpha_blend
    f = feats.to(dev)[None].requires_grad_(True)
    bgt = None if bg is None else bg.to(dev)[None]
    color, _, op, acc, bw, bgT, _ = ray_march(dist.to(dev)[None], valid.to(dev)[None], f, radiance_render, alpha_blend, bgt)
    grad, = torch.autograd.grad(color, f, g.to(dev)[None])
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    out = dict(ray_color=color[0], opacity=op[0], acc_transmission=acc[0], blend_weight=bw[0, ..., 0], background_transmission=bgT[0, :, 0])
    return {k: v.detach().cpu() for k, v in out.items()}, grad[0].detach().cpu()


def hip_case(ref, dev, g=None, rows=None):
    sel = slice(None) if rows is None else rows
    return hip_march(ref.dist[sel], ref.valid[sel], ref.feats[sel], (ref.g if g is None else g)[sel], ref.bg, dev)


def quantiles(e):
    e = np.sort(e.numpy())
    return dict(median=float(np.median(e)), p95=float(np.quantile(e, 0.95)), max=float(e[-1]))


def check_forward(ref, out):
    bad = []
    for k in FORWARD_KEYS:
        err = float((out[k].double() - ref.out64[k]).abs().max())
        o = float((ref.out32[k].double() - ref.out64[k]).abs().max())
        print("%-24s %-24s max |hip - f64| %.2e   fp32 oracle %.2e   bar %.1e%s" % (case_id(ref.case), k, err, o, FORWARD_BAR,
                                                                                    "" if err <= FORWARD_BAR else "   <-- beyond the bar"))
        assert bool(torch.isfinite(out[k]).all()), (ref.case, k)
        if not err <= FORWARD_BAR:
            bad.append((k, err))
    assert not bad, (ref.case, bad)


def check_backward(ref, grad, margin=BACKWARD_MARGIN):
    """the per-ray figures of the module's docstring: one table row per (tensor, quantile), printed before anything is asserted"""
    assert bool(torch.isfinite(grad).all()), ref.case
    E = per_ray_error(grad, ref.d64)
    bad = []
    for i, name in enumerate(("d sigma", "d rgb")):
        m = ref.counted(i)
        qh, qo = quantiles(E[i][m]), quantiles(ref.E32[i][m])
        for q in ("median", "p95", "max"):
            asserted = ref.kind != "opaque" or q == "median"
            over = asserted and not qh[q] <= margin * qo[q]
            print("%-24s %-8s E over %3d rays  %-6s hip %.2e   fp32 oracle %.2e   ratio %5.2f%s%s" % (
                case_id(ref.case), name, int(m.sum()), q, qh[q], qo[q], qh[q] / qo[q] if qo[q] > 0 else float("inf"),
                "" if asserted else "   (not asserted)", "   <-- beyond %.1f x the oracle" % margin if over else ""))
            if over:
                bad.append((name, q, qh[q], qo[q]))
        if ref.kind == "opaque" and not qh["max"] <= OPAQUE_HIP_E:
            print("%-24s %-8s E max %.2e on the counted rays   <-- beyond %.0e" % (case_id(ref.case), name, qh["max"], OPAQUE_HIP_E))
            bad.append((name, "max on counted rays", qh["max"], OPAQUE_HIP_E))
    assert not bad, (ref.case, bad)


def check_exact(ref, out, grad):
    """the bit conditions on one run of a case"""
    z = torch.zeros(())
    inv = ~ref.valid
    assert torch.equal(out["acc_transmission"][:, 0], torch.ones(R))
    assert torch.equal(out["opacity"][inv], z.expand(int(inv.sum()))) and torch.equal(out["blend_weight"][inv], z.expand(int(inv.sum())))
    assert torch.equal(grad[inv], torch.zeros(int(inv.sum()), 4)), "a gradient on an invalid slot"
    for r in ref.rows["empty"]:
        assert float(out["background_transmission"][r]) == 1.0
        assert torch.equal(out["ray_color"][r], torch.zeros(3) if ref.bg is None else ref.bg)
        assert torch.equal(grad[r], torch.zeros(ref.SR, 4))
    for r in ref.rows["zero_grad"]:
        assert torch.equal(grad[r], torch.zeros(ref.SR, 4)), "a zero-gradient ray left a non-zero gradient"


def check_scaling(ref, dev):
    """grad_color x 2^-30 and x 2^20 multiplies every gradient by exactly that power.  On the random rays of a thin case: their transmittance
    stays above 1e-3, so no product comes near the under- or overflow of fp32 (the hand-built surface rays reach 1e-36 behind the surface)."""
    assert ref.kind == "thin"
    rows = slice(0, min(sum(ref.rows.values(), [])))
    assert float(ref.out64["background_transmission"][rows].min()) > 1e-3
    _, base = hip_case(ref, dev, rows=rows)
    assert float(base.abs().max()) > 0
    for p in (-30, 20):
        _, gs = hip_case(ref, dev, g=ref.g * 2.0 ** p, rows=rows)
        assert torch.equal(gs * 2.0 ** -p, base), (ref.case, "x 2^%d" % p)


def check_ray_alone(ref, out, grad, dev, r):
    """ray r run as an R = 1 call gives the bits it has among the R rays"""
    o1, g1 = hip_case(ref, dev, rows=slice(r, r + 1))
    for k in FORWARD_KEYS:
        assert torch.equal(o1[k][0], out[k][r]), (ref.case, r, k)
    assert torch.equal(g1[0], grad[r]), (ref.case, r)


# ---- the two C entry points, called directly --------------------------------------------------------------------------------------------

def _c_calls(dev):
    from pointnerf_amd import _lib as L, ops
    return L, L.lib(), ops._ptr, ops._stream


def _carve(dev, n, dtype, pad, fill):
    """n elements in the middle of a buffer of n + 2 pad elements filled with `fill`: (buffer, view)"""
    big = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return big, big[pad:pad + n]


def check_guarded_memory(ref, out, grad, dev, pad=256):
    """The case through the two entry points, every array carved out of a larger buffer whose surroundings hold NaN (valid flags: 1, so a
    slot read beyond the ray would count): the same bits as through ray_march, and not one element written outside the arrays."""
    L, lib, ptr, stream = _c_calls(dev)
    SR, nan = ref.SR, float("nan")
    ins = {}
    for name, t, dt, fill in (("dist", ref.dist, torch.float32, nan), ("valid", ref.valid.to(torch.uint8), torch.uint8, 1),
                              ("feats", ref.feats, torch.float32, nan), ("g", ref.g, torch.float32, nan)):
        ins[name] = _carve(dev, t.numel(), dt, pad, fill)
        ins[name][1].copy_(t.flatten().to(dev))
    outs = {k: _carve(dev, n, torch.float32, pad, nan) for k, n in (("ray_color", 3 * R), ("opacity", R * SR), ("acc_transmission", R * SR),
                                                                     ("blend_weight", R * SR), ("background_transmission", R), ("grad", 4 * R * SR))}
    bg3 = None if ref.bg is None else (ctypes.c_float * 3)(*ref.bg.tolist())
    p = lambda d, k: ptr(d[k][1])
    assert lib.pnerf_raymarch_forward(p(ins, "dist"), p(ins, "valid"), p(ins, "feats"), bg3, R, SR, p(outs, "ray_color"), p(outs, "opacity"),
                                      p(outs, "acc_transmission"), p(outs, "blend_weight"), p(outs, "background_transmission"), stream()) == 0
    assert lib.pnerf_raymarch_backward(p(ins, "dist"), p(ins, "valid"), p(ins, "feats"), bg3, R, SR, p(ins, "g"), p(outs, "grad"), stream()) == 0
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    for k, (big, view) in outs.items():
        want = grad if k == "grad" else out[k]
        assert torch.equal(view.cpu(), want.flatten()), (ref.case, k, "depends on the memory around the arrays")
        assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all()), (ref.case, k, "written outside the array")


def check_return_codes(dev):
    """PNERF_E_INVAL for SR = 0, R < 0 and each null pointer; R = 0 returns 0 and touches nothing; bg3_host = NULL is legal; SR beyond the
    backward's one lane per chunk is PNERF_E_UNSUP (include/pnerf.h)"""
    L, lib, ptr, stream = _c_calls(dev)
    INVAL, UNSUP = -1, -4
    assert "PNERF_E_INVAL" in L.ERRORS[INVAL] and "PNERF_E_UNSUP" in L.ERRORS[UNSUP]
    Rn, SR, nan = 3, 5, float("nan")
    dist = torch.full((Rn, SR), 0.01, device=dev)
    valid = torch.ones(Rn, SR, dtype=torch.uint8, device=dev)
    feats = torch.ones(Rn, SR, 4, device=dev)
    g = torch.ones(Rn, 3, device=dev)
    outs = [torch.full(s, nan, device=dev) for s in ((Rn, 3), (Rn, SR), (Rn, SR), (Rn, SR), (Rn,))]
    gf = torch.full((Rn, SR, 4), nan, device=dev)
    bg3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)

    def fwd(R_=Rn, SR_=SR, bg=bg3, null=None):
        a = [ptr(dist), ptr(valid), ptr(feats)] + [ptr(o) for o in outs]
        if null is not None:
            a[null] = ptr(None)
        return lib.pnerf_raymarch_forward(a[0], a[1], a[2], bg, R_, SR_, a[3], a[4], a[5], a[6], a[7], stream())

    def bwd(R_=Rn, SR_=SR, bg=bg3, null=None):
        a = [ptr(dist), ptr(valid), ptr(feats), ptr(g), ptr(gf)]
        if null is not None:
            a[null] = ptr(None)
        return lib.pnerf_raymarch_backward(a[0], a[1], a[2], bg, R_, SR_, a[3], a[4], stream())

    untouched = lambda: all(bool(torch.isnan(t).all()) for t in outs + [gf])
    for call, n_ptr in ((fwd, 8), (bwd, 5)):
        assert call(SR_=0) == INVAL and call(SR_=-1) == INVAL and call(R_=-1) == INVAL
        for i in range(n_ptr):
            assert call(null=i) == INVAL, (call.__name__, "null pointer", i)
        assert call(R_=0) == 0
    assert bwd(SR_=4097) == UNSUP
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert untouched(), "a refused or empty call wrote to its outputs"
    assert fwd(bg=None) == 0 and bwd(bg=None) == 0
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in outs + [gf])

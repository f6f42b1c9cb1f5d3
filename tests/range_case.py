"""Gradient accuracy of DOWN-WEIGHTED rays (test infrastructure, shared by tests/test_gpu_gradient_range.py and the host-emulator twin
tests/test_gradient_range_emu.py, as mix_case.py serves the tile-GEMM tests).

The hit rays of a small pixel block are split by pixel column: group B = the right half of the block, group A = the rest, so that every
64-row tile of both backward kernels mixes rows of both groups.  The probe (ray colour x probe).sum() is multiplied by 10^-k on the B rays.
Gradients are linear in the probe: the float64 yardstick and the fp32 oracle are evaluated ONCE per case, with the probe restricted to A
and to B at weight 1, and the exact gradient at any k is gA + 10^-k gB -- on the points only B rays touch ("B-only"), 10^-k gB.

What is asserted on the B-only points is the error relative to the largest float64 gradient AMONG THOSE POINTS, not relative to the
tensor's maximum (which the A rays set): the question every other gradient bar of the suite leaves open."""
import numpy as np
import torch

import test_gpu_backward as TB
from pointnerf_amd import config, scenes, ops
from oracle import pyref

POINT_KEYS = ("points_embeding", "points_color", "points_dir", "points_conf")
EPS_KINK = 2e-6                      # float64 |pre-activation| below which a LeakyReLU unit may flip in fp32 (tests/test_gpu_bench_config.py)
BAR = {16: 1e-5, 8: 1e-4}            # the point-gradient bars of tests/test_gpu_bench_config.py: f16 cross terms, e4m3 cross terms (shipped)

# name: (K, SR, P, block size, points, scene seed, theta, MLP seed): seeds for which the fp32 ORACLE alone meets Reference.check_conditions
CASES = {
    "k8": (8, 24, 12, 12, 1500, 6, 30.0, 0),             # three sample classes: the small_k8 scale
    "k4": (4, 16, 12, 10, 900, 5, 70.0, 1),
    "k3": (3, 20, 24, 12, 2500, 0, 55.0, 3),             # the run-time-K branch of b_front
    "k12": (12, 20, 24, 12, 2500, 5, 55.0, 3),
    "emu": (8, 12, 24, 6, 1200, 11, 55.0, 3),            # the 6 x 6 block of test_emu_kernels._tiny_case(8, 12, 6, seed=11)
}


def build(name, cases=CASES):
    K, SR, P, size, n, seed, theta, mlp_seed = cases[name]
    opt = config.lego_opt(K=K, SR=SR, P=P, max_o=50000, ranges=[-0.3, -0.3, -0.3, 0.3, 0.3, 0.3])
    xyz = torch.from_numpy(scenes.chair_points(n, seed=seed, radius=0.06))
    attrs = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, 32, seed).items()}
    x0 = 400 - size // 2
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=theta, x0=x0, y0=x0, size=size))
    mlp = pyref.init_mlp_params(opt, seed=mlp_seed, bias_scale=0.1)
    return (opt, xyz, attrs, inp, mlp), x0 + size // 2


class Reference:
    """One fp32 oracle evaluation and one float64 evaluation of a case; gradients of the A and of the B part of the probe, each at weight 1."""

    def __init__(self, name):
        torch.set_num_threads(8)
        self.name = name
        self.case, xmid = build(name)
        opt, xyz, attrs, inp, mlp = self.case
        om = {k: v.clone().requires_grad_(True) for k, v in mlp.items()}
        op = dict(xyz=xyz, **{k: v.clone().requires_grad_(True) for k, v in attrs.items()})
        ref = pyref.render(opt, op, om, inp, nthreads=8)
        hit = ref["ray_mask"][0] > 0
        self.inB = inp["pixel_idx"][0][hit][:, 0] >= xmid               # [R''] hit rays of the right half of the block
        self.probe = torch.rand(ref["coarse_raycolor"].shape, generator=torch.Generator().manual_seed(123))[0]      # [R'', 3]
        assert 0 < int(self.inB.sum()) < self.inB.numel()
        kink = {}
        out64, p64, m64 = pyref.render_f64(opt, op, om, inp, ref["query"], kink=kink)
        mk, pk = list(mlp), list(attrs)

        def grads(out, pm, pp, dt):
            res = {}
            for g, sel in (("A", ~self.inB), ("B", self.inB)):
                pr = (self.probe * sel[:, None]).to(dt)
                gs = torch.autograd.grad((out["coarse_raycolor"][0] * pr).sum(), [pm[k] for k in mk] + [pp[k] for k in pk], retain_graph=True)
                res[g] = ({k: v.double() for k, v in zip(mk, gs[:len(mk)])}, {k: v[0].double() for k, v in zip(pk, gs[len(mk):])})
            return res
        self.g32, self.g64 = grads(ref, om, op, torch.float32), grads(out64, m64, p64, torch.float64)
        # the point sets
        pidx = ref["query"]["sample_pidx"][0]                           # [R'', SR, K]
        N = xyz.shape[0]
        tA, tB = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
        a, b = pidx[~self.inB], pidx[self.inB]
        tA[a[a >= 0].long()] = True
        tB[b[b >= 0].long()] = True
        b_only = tB & ~tA
        # points touched by a neighbor row / sample within EPS_KINK of a LeakyReLU kink (float64 pre-activations)
        mask = pidx >= 0
        kinked = torch.zeros(N, dtype=torch.bool)
        kinked[pidx[mask][kink["row_min_pre"] < EPS_KINK].long()] = True
        sp = pidx[mask.any(dim=-1)][kink["sample_min_pre"] < EPS_KINK]
        kinked[sp[sp >= 0].long()] = True
        self.n_kinked_rows = int((kink["row_min_pre"] < EPS_KINK).sum()) + int((kink["sample_min_pre"] < EPS_KINK).sum())
        self.touchedA, self.b_only_all, self.b_only = tA, b_only, b_only & ~kinked
        self.n_left_out = int((b_only & kinked).sum())

    def check_conditions(self):
        """conditions on the CASE, not measurements: enough B-only points, few of them lost to kinks, and the fp32 oracle inside the tightest bar"""
        n = int(self.b_only_all.sum())
        assert n >= 30, (self.name, "B-only points", n)
        assert self.n_left_out <= 0.02 * n, (self.name, "B-only points left out for kinks", self.n_left_out, n)
        for k in POINT_KEYS:
            assert self.oracle_error(k) <= BAR[16], (self.name, k, self.oracle_error(k))

    def probe_at(self, wB):
        """[R'', 3]: the probe with the B rays multiplied by wB"""
        return self.probe * torch.where(self.inB, float(wB), 1.0)[:, None].to(self.probe.dtype)

    def exact(self, wB):
        gm = {k: self.g64["A"][0][k] + wB * self.g64["B"][0][k] for k in self.g64["A"][0]}
        gp = {k: self.g64["A"][1][k] + wB * self.g64["B"][1][k] for k in self.g64["A"][1]}
        return gm, gp

    def oracle_error(self, key):
        """the fp32 oracle's own error on the B-only points, relative to their largest float64 gradient (the same at every k: floating point)"""
        b = self.g64["B"][1][key][self.b_only]
        return float((self.g32["B"][1][key][self.b_only] - b).abs().max()) / float(b.abs().max())


def hip_backward(ref, ctx, dense, fwd, probe_hit):
    """one backward of the HIP path on a finished forward: (MLP gradients, point gradients) as float64 CPU tensors"""
    opt = ref.case[0]
    dev = ctx["raydir"].device
    hit = dense["ray_hit"] > 0
    g = torch.zeros(ctx["R"], 3, device=dev)
    g[hit] = probe_hit.float().to(dev)
    gflat = torch.zeros_like(ctx["flat"])
    grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
    ops.render_backward(ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], fwd, g, gflat, grads)
    torch.cuda.synchronize()
    lay, _ = ops.mlp_layout()
    return ({k: gflat[o:o + int(np.prod(shp))].view(shp).cpu().double() for k, (o, shp) in lay.items()}, {k: v.cpu().double() for k, v in grads.items()})


def group_errors(ref, gp, wB, scale=1.0):
    """per point tensor: max |hip / scale - f64| over the B-only points, relative to the largest |f64| among them"""
    out = {}
    for k in POINT_KEYS:
        b = wB * ref.g64["B"][1][k][ref.b_only]
        out[k] = float((gp[k][ref.b_only] / scale - b).abs().max()) / float(b.abs().max())
    return out


def check_rest(ref, gm, gp, wB, scale=1.0):
    """the A-touched points and every MLP tensor keep the bars of tests/test_gpu_backward.py::_check (per tensor maximum), whatever the B rows do"""
    em, ep = ref.exact(wB)
    for k in em:
        assert bool(torch.isfinite(gm[k]).all()), k
        TB._check(k, (gm[k] / scale).float(), em[k].float())
    for k in POINT_KEYS:
        assert bool(torch.isfinite(gp[k]).all()), k
        TB._check(k + "[A]", (gp[k][ref.touchedA] / scale).float(), ep[k][ref.touchedA].float())


def report(ref, tag, wB, errs, bar):
    """one table row per tensor: the HIP figure, the fp32 oracle's own beside it; returns the tensors beyond the bar"""
    bad = []
    for k in POINT_KEYS:
        o = ref.oracle_error(k)
        print("%-5s %-22s weight of B %-9.3g %-16s |hip - f64| / max|f64| over the %d B-only points: %.2e   fp32 oracle %.2e   bar %.0e%s" %
              (ref.name, tag, wB, k, int(ref.b_only.sum()), errs[k], o, bar, "" if errs[k] <= bar else "   <-- beyond the bar"))
        if not errs[k] <= bar:
            bad.append((k, errs[k]))
    return bad


def run_arithmetic(ref, render, bits, ks, extras=True, tag=None):
    """One forward with the cross terms of the input-gradient chain set to `bits`, then one backward per k in ks (the B rays at 10^-k) and, with
    `extras`, the whole-call scales 2^-30 / 2^+20 of the k = 0 probe and the exact-zero probe on the B rays.  Every assertion of the module's
    docstring; the figures are printed before anything is asserted."""
    tag = tag or ("f16 cross terms" if bits == 16 else "e4m3 cross terms")
    bar = BAR[bits]
    old_bits, _ = ops.set_cross_terms(bits)
    try:
        dense, fwd, ctx = render(*ref.case, train=True)
        failures = []
        for k in ks:
            wB = 10.0 ** -k
            gm, gp = hip_backward(ref, ctx, dense, fwd, ref.probe_at(wB))
            failures += [(k,) + b for b in report(ref, tag + ", k = %d" % k, wB, group_errors(ref, gp, wB), bar)]
            check_rest(ref, gm, gp, wB)
        if extras:
            for p in (-30, 20):
                s = 2.0 ** p
                gm, gp = hip_backward(ref, ctx, dense, fwd, ref.probe_at(1.0) * s)
                failures += [("2^%d" % p,) + b for b in report(ref, tag + ", x 2^%d" % p, 1.0, group_errors(ref, gp, 1.0, s), bar)]
                check_rest(ref, gm, gp, 1.0, s)
            gm, gp = hip_backward(ref, ctx, dense, fwd, ref.probe_at(0.0))
            check_rest(ref, gm, gp, 0.0)
            for k in POINT_KEYS:          # a ray whose probe is exactly 0 contributes exactly 0
                assert float(gp[k][ref.b_only_all].abs().max()) == 0.0, (k, "a zero-gradient ray left a non-zero gradient")
        assert not failures, failures
    finally:
        ops.set_cross_terms(old_bits)

"""The forward has no atomics: the same inputs must give the same bits, launch after launch.  Round 3 found that they did not -- in 1.1 % of
the launches ONE sample's aggregated feature row was off in 16 columns (its RGB by ~1e-2, far outside the 1e-4 bar), always the low
register of a v_pk_fma_f32 pair for one 16-lane pass: dependent packed-fp32 FMA chains the compiler had formed in the forward's tail
(csrc/Makefile: the library is built without the vectorisers since; tests/test_boundary.py checks the disassembly).  This test repeats
the inference forward of the configs[1] subsample through the C ABI and compares the colour MLP's input rows (the workspace's first
region) and the decoded samples bit for bit: 400 launches caught the old build with probability 0.99."""
import ctypes

import pytest
import torch

from pointnerf_amd import ops, _lib as L
from pointnerf_amd.point_query import lighting_fast_querier
from test_gpu_bench_config import _bench_case

pytestmark = pytest.mark.gpu
LAUNCHES = 400


def test_inference_forward_is_bit_reproducible():
    opt, xyz, attrs, inp, mlp = _bench_case()
    dev = torch.device("cuda:0")
    xyz_d = xyz.to(dev).contiguous()
    pts_t = {k: v.detach().to(dev).reshape(v.shape[1], v.shape[2]).contiguous() for k, v in attrs.items()}
    raydir = inp["raydir"][0].to(dev).contiguous()
    dense = lighting_fast_querier(dev, opt).query_dense(xyz_d[None], xyz.shape[0], float(inp["near"].min()), float(inp["far"].max()), raydir[None],
                                                        inp["campos"].to(dev))
    n_valid = int(dense["counters"][0].item())
    flat = ops.flatten_mlp(mlp, dev)
    packed = ops.pack_mlp(flat)
    cam = ops.make_camera(inp["campos"][0].numpy(), inp["camrotc2w"][0].numpy(), opt.vsize[2], opt.raydist_mode_unit, bg=inp["bg_color"][0].numpy())
    pts = ops.make_points(xyz_d, pts_t["points_embeding"], pts_t["points_conf"], pts_t["points_dir"], pts_t["points_color"])
    R, SR, K = raydir.shape[0], opt.SR, opt.K
    lib = L.lib()
    f32 = dict(dtype=torch.float32, device=dev)
    nws = lib.pnerf_agg_workspace_bytes(n_valid, K)
    decoded, weight = torch.empty(R, SR, 4, **f32), torch.empty(R, SR, K, **f32)
    ray_color, opacity, bg_trans, blend_w = torch.empty(R, 3, **f32), torch.empty(R, SR, **f32), torch.empty(R, **f32), torch.empty(R, SR, **f32)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    step = ops.make_step(raydir, dense, flat, packed, R, SR, K, n_valid)
    first, differing = None, []
    for it in range(LAUNCHES):
        ws.fill_(0xFF)                                    # (NaN patterns: nothing may be read that this launch did not write)
        L.check(lib.pnerf_render_forward(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(step),
                                         ops._ptr(decoded), ops._ptr(weight), ops._ptr(ray_color), ops._ptr(opacity), ops._ptr(bg_trans), ops._ptr(blend_w),
                                         None, ops._ptr(ws), nws, ops._stream()), "pnerf_render_forward")
        cur = (ws[: n_valid * 256 * 4].clone(), decoded.clone(), ray_color.clone())           # f rows (bytes), decoded, ray colours
        if first is None:
            first = cur
            assert bool(torch.isfinite(decoded).all()) and float(decoded.abs().max()) > 0.0
        elif not all(torch.equal(a, b) for a, b in zip(cur, first)):
            differing.append(it)
    assert not differing, "launches whose forward differs from the first one's: %s" % differing[:10]


def test_training_forward_and_its_saved_activations_are_bit_reproducible():
    """the same for the training forward: outputs AND every byte it saves for the backward (k-major planes written through the LDS transpose
    read and v_pk_add_f16, sign words, row metadata, h4 rows, class lists) -- the arena is pre-filled with 0xFF, so bytes the launch does
    not write compare equal too"""
    from gpu_util import hip_render
    opt, xyz, attrs, inp, mlp = _bench_case()
    first, differing = None, []
    for it in range(150):
        dense, fwd, ctx = hip_render(opt, xyz, attrs, inp, mlp, train=True)          # (conftest: Arena.take fills the block with 0xFF)
        need = L.lib().pnerf_agg_saved_bytes(ctx["n_valid"], opt.K)
        cur = (fwd["saved"][:need].clone(), fwd["decoded"].clone(), fwd["ray_color"].clone())
        ops.ARENA.give(fwd["saved"])
        if first is None:
            first = cur
        elif not all(torch.equal(a, b) for a, b in zip(cur, first)):
            differing.append(it)
    assert not differing, "launches whose training forward differs from the first one's: %s" % differing[:10]


def test_backward_chain_and_weight_gradient_gemms_are_bit_reproducible():
    """the backward adds the POINT gradients (and the small head / bias sums) with atomics -- those differ in the last bits from run to run --
    but its dgrad chain and the split-K weight-gradient GEMMs are deterministic: the output-gradient planes it saves and d W of the seven MFMA
    layers (and the four aggregator bias gradients, the GEMMs' ones column) must be the same bits, launch after launch"""
    import numpy as np
    from gpu_util import hip_render, DEV
    opt, xyz, attrs, inp, mlp = _bench_case()
    dev = torch.device(DEV)
    lay, _ = ops.mlp_layout()
    det = [k for k in lay if k in ("block1.0.weight", "block1.0.bias", "block1.2.weight", "block1.2.bias", "block3.0.weight", "block3.0.bias",
                                   "block3.2.weight", "block3.2.bias", "color_branch.0.weight", "color_branch.2.weight", "color_branch.4.weight")]
    assert len(det) == 11
    probe = torch.rand(768, 3, generator=torch.Generator().manual_seed(123)).to(dev)
    first, differing = None, []
    for it in range(80):
        dense, fwd, ctx = hip_render(opt, xyz, attrs, inp, mlp, train=True)
        hit = dense["ray_hit"] > 0
        g = torch.zeros(ctx["R"], 3, device=dev)
        g[hit] = probe[: int(hit.sum())]
        gflat = torch.zeros_like(ctx["flat"])
        grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
        ops.render_backward(ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], fwd, g, gflat, grads)
        need = L.lib().pnerf_agg_saved_bytes(ctx["n_valid"], opt.K)
        cur = [fwd["saved"][:need].clone()] + [gflat[lay[k][0]: lay[k][0] + int(np.prod(lay[k][1]))].clone() for k in det]
        ops.ARENA.give(fwd["saved"])
        if first is None:
            first = cur
            assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in cur[1:])
        else:
            bad = [(["saved area"] + det)[i] for i, (a, b) in enumerate(zip(cur, first)) if not torch.equal(a, b)]
            if bad:
                differing.append((it, bad))
    assert not differing, differing[:5]

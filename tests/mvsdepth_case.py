"""Depth maps from images (csrc/mvsdepth.hip, pointnerf_amd/depth_estimators.py, the mode-1 shell) -- the cases, float64 restatements and
checks shared by the device suite (tests/test_gpu_mvsdepth.py) and the host emulator (tests/test_mvsdepth_emu.py).

Inputs are regenerated here from numpy generators (identical everywhere); the fixture tests/golden/refmvsdepth.npz holds what the
reference's own lines compute from them on CPU float32 (tests/golden/make_mvsdepth_golden.py: homo_warping and the variance lines, MVSNet's
tail, the sampler lines, MVSNet and the pyramid FeatureNet end to end) and the MARGINS: per case and quantity, the reference's own largest
fp32 deviation from the float64 restatement of this file.  Every bar below is four times that number; none is
tuned to the kernels.  Network weights are not stored: `fill_weights` fills any state_dict key by key from a generator seeded with the seed
and a hash of the key, for the reference's modules and this package's alike.

The expected depth INDEX is a hard decision (`.long()` truncates): a pixel is decided where the float64 index lies farther from an integer
than the index margin; on decided pixels the confidence window must be the float64 one, and at most 1 % of a case's pixels may be undecided."""
import os
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "refmvsdepth.npz")
UNDECIDED_CAP = 0.01
WILD = 1e6                          # float64 sample coordinates beyond this (or non-finite) are not compared with the reference

_fx = None


def fixture():
    global _fx
    if _fx is None:
        with np.load(FIX) as z:
            _fx = {k: z[k] for k in z.files}
    return _fx


def bar(name):
    """four times the reference's own fp32 deviation recorded in the fixture"""
    v = float(fixture()["dev_" + name])
    assert v > 0, "margin %s not recorded" % name
    return 4.0 * v


def fill_weights(module, seed):
    """Fills every state_dict entry in place, key by key, from default_rng([seed, crc32(key)]): convolution weights N(0, 2 / fan_in) (the
    activations keep their scale through the ReLUs), the last 3-D convolution `prob` six times that (the logits then spread over several units
    and the probability volume is not flat), norm scales U(0.8, 1.2), running means N(0, 0.1^2), running variances U(0.5, 1.5), biases
    N(0, 0.1^2)."""
    sd = module.state_dict()
    for key, t in sd.items():
        rng = np.random.default_rng([seed, zlib.crc32(key.encode())])
        shape = tuple(t.shape)
        if key.endswith("num_batches_tracked"):
            v = np.zeros(shape)
        elif key.endswith("running_mean"):
            v = rng.normal(0.0, 0.1, shape)
        elif key.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif key.endswith("bias"):
            v = rng.normal(0.0, 0.1, shape)
        elif len(shape) == 1:
            v = rng.uniform(0.8, 1.2, shape)
        else:
            fan = int(np.prod(shape[1:]))
            if any(s in key for s in ("conv7.0", "conv9.0", "conv11.0")):           # transposed, stride 2: an output sees 1 / 8 of the taps
                fan = shape[0] * int(np.prod(shape[2:])) / 8.0
            v = rng.normal(0.0, np.sqrt(2.0 / fan), shape) * (6.0 if ".prob." in "." + key else 1.0)
        with torch.no_grad():
            t.copy_(torch.from_numpy(np.asarray(v)).to(t.dtype))
    module.load_state_dict(sd)
    return module


# ---- 1. cost volume -------------------------------------------------------------------------------------------------------------------------
CV_CASES = {"shift": dict(B=1, V=3, D=5, h=13, w=37, ac=False, seed=101, turned=None),
            "shared_ac": dict(B=2, V=3, D=3, h=9, w=21, ac=True, seed=102, turned=None),
            "behind": dict(B=1, V=3, D=4, h=9, w=21, ac=False, seed=103, turned=2)}


def _rot_y(a):
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def cv_inputs(name):
    """-> feats [V,32,h,w] f32 (one set for every batch item), proj [B,V,4,4] f32 (view 0 the identity, the others K [R|t] K^-1 with a shift
    of several pixels; view `turned` faces away: its z is zero in one image column and negative beyond it), depth_values [B,D] f32"""
    c = CV_CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, V, D, h, w = c["B"], c["V"], c["D"], c["h"], c["w"]
    feats = rng.standard_normal((V, 32, h, w)).astype(np.float32)
    K = np.array([[float(w), 0.0, (w - 1) / 2.0], [0.0, float(w), (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    proj = np.zeros((B, V, 4, 4))
    for b in range(B):
        for v in range(V):
            R = _rot_y(0.05 * v * (1 + b))
            t = np.array([0.3 * v, -0.2 * v, 0.05 * v]) * (1 + 0.5 * b)
            proj[b, v, :3, :3] = K @ R @ np.linalg.inv(K)
            proj[b, v, :3, 3] = K @ t
            proj[b, v, 3, 3] = 1.0
            if v == c["turned"]:
                # z = (1 - x / 8) depth in exactly representable numbers: 0 in column 8 (x / 0, 0 / 0 ...), negative beyond it, and
                # coordinates of tens to thousands of pixels next to it
                proj[b, v, :3] = [[1.0, 0.0, 3.0, 0.5], [0.0, 1.0, 0.5, 0.25], [-0.125, 0.0, 1.0, 0.0]]
    dv = np.stack([np.linspace(2.0 + 0.3 * b, 4.0 + 0.3 * b, D) for b in range(B)])
    return feats, proj.astype(np.float32), dv.astype(np.float32), c["ac"]


def cost_volume64(feats, proj, dv, align_corners):
    """module.py:47-66 and mvsnet.py:110-122 in float64 on the float32 inputs -> (variance [B,32,D,h,w], wild [B,D,h,w] bool: some view's
    sample coordinate is non-finite or beyond WILD there; such a view contributes zero taps)"""
    feats, proj, dv = feats.astype(np.float64), proj.astype(np.float64), dv.astype(np.float64)
    V, C, h, w = feats.shape
    B, D = dv.shape
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pix = np.stack([xs.ravel(), ys.ravel(), np.ones(h * w)])
    var = np.zeros((B, C, D, h, w))
    wild = np.zeros((B, D, h, w), bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            s1, s2 = np.zeros((C, D, h * w)), np.zeros((C, D, h * w))
            for v in range(V):
                rot_xyz = proj[b, v, :3, :3] @ pix                                            # [3,hw]
                p = rot_xyz[:, None, :] * dv[b][None, :, None] + proj[b, v, :3, 3][:, None, None]      # [3,D,hw]
                gx = (p[0] / p[2]) / ((w - 1) / 2) - 1
                gy = (p[1] / p[2]) / ((h - 1) / 2) - 1
                if align_corners:
                    ix, iy = (gx + 1) / 2 * (w - 1), (gy + 1) / 2 * (h - 1)
                else:
                    ix, iy = ((gx + 1) * w - 1) / 2, ((gy + 1) * h - 1) / 2
                bad = ~(np.isfinite(ix) & np.isfinite(iy) & (np.abs(ix) <= WILD) & (np.abs(iy) <= WILD))
                wild[b] |= bad.reshape(D, h, w)
                ixs, iys = np.where(bad, -10.0, ix), np.where(bad, -10.0, iy)                 # no tap inside
                x0, y0 = np.floor(ixs), np.floor(iys)
                s = np.zeros((C, D, h * w))
                for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    xx, yy = x0 + dx, y0 + dy
                    wgt = (1 - np.abs(ixs - xx)) * (1 - np.abs(iys - yy))
                    ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                    xi, yi = np.clip(xx, 0, w - 1).astype(np.int64), np.clip(yy, 0, h - 1).astype(np.int64)
                    s += feats[v][:, yi, xi] * np.where(ok, wgt, 0.0)[None]
                s1 += s
                s2 += s * s
            var[b] = (s2 / V - (s1 / V) ** 2).reshape(C, D, h, w)
    return var, wild


def check_cost_volume(name, dev):
    from pointnerf_amd import ops
    feats, proj, dv, ac = cv_inputs(name)
    fx = fixture()
    t = lambda a: torch.from_numpy(a).to(dev)
    got = ops.mvs_cost_volume(t(feats), t(proj), t(dv), align_corners=ac)
    again = ops.mvs_cost_volume(t(feats), t(proj), t(dv), align_corners=ac)
    B, D = dv.shape
    assert got.shape == (B, 32, D) + feats.shape[2:] and got.dtype == torch.float32
    assert torch.equal(got, again), "two calls differ"
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    want, wild = cost_volume64(feats, proj, dv, ac)
    scale = float((feats.astype(np.float64) ** 2).max())
    err = np.abs(got - want).max() / scale
    print(name, "variance err / max feat^2 = %.3e (bar %.3e), wild voxels %d of %d" % (err, bar("cv_" + name), wild.sum(), wild.size))
    assert err <= bar("cv_" + name)                       # everywhere: a wild view's taps are exactly zero in the restatement
    if CV_CASES[name]["turned"] is not None:
        assert 0 < wild.sum() < wild.size
    else:
        assert not wild.any()
    tame = ~np.broadcast_to(wild[:, None], got.shape)
    ref = fx["cv_%s_var" % name].astype(np.float64)
    err_fx = np.abs(got - ref)[tame].max() / scale
    print(name, "against the reference fixture %.3e" % err_fx)
    assert err_fx <= 2 * bar("cv_" + name)                # both sides within their own deviation of float64
    # the B = 2 case shares one feature set: handing the same maps over per batch item changes nothing
    if B > 1:
        per_item = ops.mvs_cost_volume(t(np.broadcast_to(feats, (B,) + feats.shape).copy()), t(proj), t(dv), align_corners=ac)
        assert np.array_equal(per_item.cpu().numpy(), got.astype(np.float32))
    # the other un-normalisation is really another result
    other = ops.mvs_cost_volume(t(feats), t(proj), t(dv), align_corners=not ac).cpu().numpy()
    assert np.abs(other - got).max() / scale > 100 * bar("cv_" + name)


# ---- 2. depth regression ------------------------------------------------------------------------------------------------------------------
RG_CASES = {"d16": dict(B=2, D=16, h=16, w=24, seed=201), "d192": dict(B=1, D=192, h=8, w=8, seed=202)}


def rg_inputs(name):
    """logits N(0, 3^2); in d16 the first row of batch item 0 holds +-80 (exp(80) overflows fp32 without the max-subtraction)"""
    c = RG_CASES[name]
    rng = np.random.default_rng(c["seed"])
    logits = (3.0 * rng.standard_normal((c["B"], c["D"], c["h"], c["w"]))).astype(np.float32)
    if name == "d16":
        logits[0, :, 0, :] = np.where(rng.uniform(size=(c["D"], c["w"])) < 0.5, -80.0, 80.0)
    dv = np.stack([np.linspace(2.0 + b, 6.0 + b, c["D"]) for b in range(c["B"])]).astype(np.float32)
    return logits, dv


def regress64(logits, dv):
    """mvsnet.py:127-136 in float64 -> depth [B,h,w], index (before truncation) [B,h,w], confidence [B,h,w], prob [B,D,h,w]"""
    l, dv = logits.astype(np.float64), dv.astype(np.float64)
    B, D = dv.shape
    with np.errstate(all="ignore"):
        e = np.exp(l - l.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        depth = (p * dv[:, :, None, None]).sum(1)
        fi = (p * np.arange(D, dtype=np.float64)[None, :, None, None]).sum(1)
        idx = np.clip(np.nan_to_num(np.trunc(fi)), 0, D - 1).astype(np.int64)
        pad = np.pad(p, ((0, 0), (1, 2), (0, 0), (0, 0)))
        conf = sum(np.take_along_axis(pad, (idx + k)[:, None], 1)[:, 0] for k in range(4))      # padded index idx + 1 + (k - 1)
    return depth, fi, conf, p


def decided(fi, tau):
    return np.abs(fi - np.round(fi)) > tau


def check_regress_against(depth, conf, prob, logits, dv, tag, what=""):
    """the shared assertions on (depth, confidence, prob) arrays against float64; the bars are dev_<tag>_*"""
    d64, fi, c64, p64 = regress64(logits, dv)
    ok = decided(fi, bar(tag + "_idx"))
    und = 1.0 - ok.mean()
    e_d, e_c = np.abs(depth - d64).max(), np.abs(conf - c64)[ok].max()
    print(tag, what, "depth err %.3e (bar %.3e), confidence err on decided %.3e (bar %.3e), undecided %.3f %%"
          % (e_d, bar(tag + "_depth"), e_c, bar(tag + "_conf"), 100 * und))
    assert und <= UNDECIDED_CAP
    assert e_d <= bar(tag + "_depth")
    assert e_c <= bar(tag + "_conf")                     # a window one slot off differs by a whole probability
    if prob is not None:
        e_p = np.abs(prob - p64).max()
        print(tag, what, "prob err %.3e (bar %.3e)" % (e_p, bar(tag + "_prob")))
        assert e_p <= bar(tag + "_prob")


def check_regress(name, dev):
    from pointnerf_amd import ops
    logits, dv = rg_inputs(name)
    t = lambda a: torch.from_numpy(a).to(dev)
    depth, conf = ops.mvs_depth_regress(t(logits), t(dv))
    depth2, conf2, prob = ops.mvs_depth_regress(t(logits), t(dv), return_prob=True)
    assert torch.equal(depth, depth2) and torch.equal(conf, conf2), "two calls differ"
    assert depth.shape == conf.shape == (logits.shape[0],) + logits.shape[2:] and prob.shape == logits.shape
    depth, conf, prob = (a.cpu().numpy().astype(np.float64) for a in (depth, conf, prob))
    assert np.isfinite(depth).all() and np.isfinite(conf).all() and np.isfinite(prob).all()
    check_regress_against(depth, conf, prob, logits, dv, "rg_" + name)
    fx = fixture()
    _, fi, _, _ = regress64(logits, dv)
    ok = decided(fi, bar("rg_%s_idx" % name))
    assert np.abs(depth - fx["rg_%s_depth" % name]).max() <= 2 * bar("rg_%s_depth" % name)
    assert np.abs(conf - fx["rg_%s_conf" % name])[ok].max() <= 2 * bar("rg_%s_conf" % name)
    if name == "d16":                                   # the +-80 row: uniform over its +80 entries
        n_hi = (logits[0, :, 0, :] > 0).sum(0)
        assert np.allclose(prob[0, :, 0, :].max(0), 1.0 / n_hi, rtol=1e-5)


def check_regress_nan(dev):
    """a NaN logit gives a NaN depth at its pixel, nothing else moves, nothing is read out of range"""
    from pointnerf_amd import ops
    logits, dv = rg_inputs("d16")
    clean = ops.mvs_depth_regress(torch.from_numpy(logits).to(dev), torch.from_numpy(dv).to(dev))
    bad = logits.copy()
    bad[1, 5, 7, 11] = np.nan
    bad[0, 15, 3, 2] = np.inf
    depth, conf = ops.mvs_depth_regress(torch.from_numpy(bad).to(dev), torch.from_numpy(dv).to(dev))
    d, c = depth.cpu().numpy(), conf.cpu().numpy()
    assert np.isnan(d[1, 7, 11]) and np.isnan(d[0, 3, 2])
    hit = np.zeros(d.shape, bool)
    hit[1, 7, 11] = hit[0, 3, 2] = True
    assert np.array_equal(d[~hit], clean[0].cpu().numpy()[~hit]) and np.array_equal(c[~hit], clean[1].cpu().numpy()[~hit])


# ---- 3. depth to points --------------------------------------------------------------------------------------------------------------------
DP_CASES = {"x4": dict(h=16, w=24, H=64, W=96, seed=301), "odd": dict(h=13, w=37, H=50, W=150, seed=302)}
DP_NEAR_FAR = (2.0, 6.0)


def dp_inputs(name):
    c = DP_CASES[name]
    rng = np.random.default_rng(c["seed"])
    depth = rng.uniform(DP_NEAR_FAR[0] - 0.8, DP_NEAR_FAR[1] + 0.8, (c["h"], c["w"])).astype(np.float32)
    depth[0, 0], depth[0, 1], depth[1, 0] = DP_NEAR_FAR[0], DP_NEAR_FAR[1], np.nextafter(np.float32(DP_NEAR_FAR[0]), np.float32(0))
    conf = rng.uniform(0.0, 1.0, (c["h"], c["w"])).astype(np.float32)
    K = np.array([[1.1 * c["W"], 0.0, c["W"] / 2.0 - 0.7], [0.0, 1.07 * c["W"], c["H"] / 2.0 + 0.4], [0.0, 0.0, 1.0]], np.float32)
    return depth, conf, K, (c["H"], c["W"])


def nearest_index(n_in, n_out):
    """F.interpolate(mode='nearest')'s source index: min(floor(dst * ((float)in / out)), in - 1), fp32"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def points64(depth, conf, K, size):
    """mvs_points_model.py:329-337, 152-157, 171-182 and mvs_utils.py:92-98 in float64 on the float32 inputs"""
    H, W = size
    near, far = (np.float64(np.float32(v)) for v in DP_NEAR_FAR)
    iy, ix = nearest_index(depth.shape[0], H), nearest_index(depth.shape[1], W)
    d = depth.astype(np.float64)[iy][:, ix]
    mask = (d >= near) & (d <= far)
    ndc = np.clip((d - near) / (far - near), 0.0, 1.0)
    z = ndc * (far - near) + near
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.stack([xs * z, ys * z, z], -1) @ np.linalg.inv(K.astype(np.float64).T)
    return cam, conf[iy][:, ix], mask


def check_points(name, dev):
    from pointnerf_amd import ops
    depth, conf, K, size = dp_inputs(name)
    t = lambda a: torch.from_numpy(a).to(dev)
    xyz, cf, mask = ops.depth_to_cam_points(t(depth), t(conf), size, DP_NEAR_FAR, torch.from_numpy(K))
    xyz2, cf2, mask2 = ops.depth_to_cam_points(t(depth), t(conf), size, DP_NEAR_FAR, torch.from_numpy(K))
    H, W = size
    assert xyz.shape == (1, 1, 1, H, W, 3) and cf.shape == (1, 1, H, W) and mask.shape == (1, 1, H, W) and mask.dtype == torch.bool
    assert torch.equal(xyz, xyz2) and torch.equal(cf, cf2) and torch.equal(mask, mask2), "two calls differ"
    want, cf64, m64 = points64(depth, conf, K, size)
    fx = fixture()
    assert np.array_equal(cf[0, 0].cpu().numpy(), cf64), "nearest-neighbour indices differ"
    assert np.array_equal(cf[0, 0].cpu().numpy(), fx["dp_%s_conf" % name])            # F.interpolate's own choice
    assert np.array_equal(mask[0, 0].cpu().numpy(), m64) and np.array_equal(m64, fx["dp_%s_mask" % name].astype(bool))
    assert 0.1 < m64.mean() < 0.9                                                     # depths on both sides of near and far
    err = np.abs(xyz[0, 0, 0].cpu().numpy().astype(np.float64) - want).max()
    print(name, "cam_xyz err %.3e (bar %.3e)" % (err, bar("dp_" + name)))
    assert err <= bar("dp_" + name)
    assert np.abs(xyz[0, 0, 0].cpu().numpy() - fx["dp_%s_xyz" % name]).max() <= 2 * bar("dp_" + name)


# ---- refusals of the three entry points ------------------------------------------------------------------------------------------------------
def check_entry_point_errors(dev):
    import ctypes
    import pytest
    from pointnerf_amd import ops, _lib as L
    lib = L.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    one, z = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(0)                      # a valid pointer: nothing is launched on a refusal
    cv = lambda B=1, V=2, C=32, D=2, h=4, w=4, sets=1, out=one, ws=1 << 20: lib.pnerf_mvs_cost_volume(one, sets, one, one, B, V, C, D, h, w, 0, out, one, ws, z)
    assert cv(C=16) == -4 and cv(V=0) == -1 and cv(D=0) == -1 and cv(h=1) == -1 and cv(w=1) == -1 and cv(out=z) == -1
    assert cv(B=2, sets=3) == -1 and cv(ws=16) == -2
    assert lib.pnerf_mvs_cost_volume_workspace_bytes(1, 2, 4, 4) == 2 * 32 * 16 * 4 and lib.pnerf_mvs_cost_volume_workspace_bytes(1, 0, 4, 4) == 0
    assert lib.pnerf_mvs_depth_regress(one, one, 1, 0, 4, 4, one, one, z, z) == -1
    assert lib.pnerf_mvs_depth_regress(one, one, 1, 2, 4, 4, z, one, z, z) == -1
    m = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert lib.pnerf_depth_to_cam_points(one, one, 4, 4, 1, 8, 2.0, 6.0, m, one, one, one, z) == -1
    assert lib.pnerf_depth_to_cam_points(one, one, 4, 4, 8, 8, 2.0, 6.0, None, one, one, one, z) == -1
    feats, proj, dv, _ = cv_inputs("shift")
    t = lambda a: torch.from_numpy(a).to(dev)
    with pytest.raises(RuntimeError, match="PNERF_E_UNSUP"):
        ops.mvs_cost_volume(t(feats[:, :16].copy()), t(proj), t(dv))
    with pytest.raises(ValueError, match="proj"):
        ops.mvs_cost_volume(t(feats), t(proj[:, :2].copy()), t(dv))


def check_cpu_tensors_refused():
    import pytest
    from pointnerf_amd import ops, point_init
    from pointnerf_amd.depth_estimators import MVSNet
    feats, proj, dv, _ = cv_inputs("shift")
    t = torch.from_numpy
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mvs_cost_volume(t(feats), t(proj), t(dv))
    logits, dv2 = rg_inputs("d16")
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.mvs_depth_regress(t(logits), t(dv2))
    depth, conf, K, size = dp_inputs("x4")
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.depth_to_cam_points(t(depth), t(conf), size, DP_NEAR_FAR, t(K))
    net = MVSNet()
    with torch.no_grad(), pytest.raises(RuntimeError, match="device tensor"):
        net(torch.zeros(1, 3, 3, 32, 32), torch.eye(4).expand(1, 3, 4, 4), torch.ones(1, 8))
    with torch.no_grad(), pytest.raises(RuntimeError, match="device tensor"):
        point_init.depth_maps_from_images(net, torch.zeros(3, 3, 32, 32), torch.eye(3).expand(3, 3, 3), torch.eye(4).expand(3, 4, 4),
                                          [[0, 1, 2]] * 3, (2.0, 6.0), n_depth=8)


# ---- 4. end to end through MVSNet.forward -------------------------------------------------------------------------------------------------------
E2E = dict(B=2, V=3, H=64, W=96, D=16, seed=401, wseed=7)
PYR = dict(V=2, H=16, W=24, seed=402, wseed=8)


def e2e_inputs():
    """images [B,V,3,H,W] of smooth random texture warped by the cameras' own plane homography (the views agree on a fronto-parallel plane
    at depth 3.2), proj [B,V,4,4] at feature resolution, depth_values [B,D]"""
    c = E2E
    rng = np.random.default_rng(c["seed"])
    B, V, H, W, D = c["B"], c["V"], c["H"], c["W"], c["D"]
    h, w = H // 4, W // 4
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    waves = [(rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.uniform(0, 6.28), rng.uniform(0.3, 1.0)) for _ in range(12)]

    def texture(x, y, ch):
        return sum(a * np.sin(fx * x + fy * y + ph + ch) for fx, fy, ph, a in waves) / 3.0

    Kf = np.array([[float(w), 0.0, (w - 1) / 2.0], [0.0, float(w), (h - 1) / 2.0], [0.0, 0.0, 1.0]])
    imgs, proj = np.zeros((B, V, 3, H, W)), np.zeros((B, V, 4, 4))
    for b in range(B):
        for v in range(V):
            t = np.array([0.25 * v * (1 + 0.4 * b), -0.1 * v, 0.0])
            proj[b, v, :3, :3], proj[b, v, :3, 3], proj[b, v, 3, 3] = np.eye(3), Kf @ t, 1.0
            shift = 4.0 * (Kf @ t)[:2] / 3.2                                         # image pixels at the plane's depth
            for ch in range(3):
                imgs[b, v, ch] = texture(xs - shift[0], ys - shift[1], 2.1 * ch)
    dv = np.stack([np.linspace(2.0, 5.0, D) + 0.1 * b for b in range(B)])
    return imgs.astype(np.float32), proj.astype(np.float32), dv.astype(np.float32)


def pyr_inputs():
    rng = np.random.default_rng(PYR["seed"])
    return rng.uniform(-1.0, 1.0, (1, PYR["V"], 3, PYR["H"], PYR["W"])).astype(np.float32)


def mvsnet64(net, imgs, proj, dv, align_corners=False):
    """MVSNet.forward in float64 on the CPU: `net`'s own convolutions (a float64 copy) around the restatements above -> depth, index,
    confidence, prob, cost_reg (all numpy float64)"""
    import copy
    n64 = copy.deepcopy(net).cpu().double().eval()
    with torch.no_grad():
        x = torch.from_numpy(imgs).double()
        B, V = x.shape[:2]
        feats = torch.stack([n64.feature(x[:, v]) for v in range(V)], 1).numpy()      # [B,V,32,h,w]
        var = np.concatenate([cost_volume64(feats[b], proj[b:b + 1].astype(np.float64), dv[b:b + 1].astype(np.float64), align_corners)[0]
                              for b in range(B)])
        cost = n64.cost_regularization(torch.from_numpy(var)).squeeze(1).numpy()
    return regress64(cost, dv.astype(np.float64)) + (cost,)


def pyramid64(net, imgs):
    """the pyramid's own convolutions in float64 on the CPU -> the four levels (numpy)"""
    import copy
    with torch.no_grad():
        return [l.numpy() for l in copy.deepcopy(net).cpu().double().eval()(torch.from_numpy(imgs).double())]


def make_opt(**kw):
    """the options of the reference's lego script that the mode-1 shell and gen_points read"""
    o = dict(mode=1, is_train=False, gpu_ids=[0], checkpoints_dir="", name="mvsdepth", resume_iter="best", resume_dir="", manual_depth_view=1,
             pre_d_est=None, manual_std_depth=0.0, far_plane_shift=None, depth_vid="01", init_view_num=3, depth_occ=0, ref_vid=0,
             shading_feature_mlp_layer0=0, num_each_depth=1, mvs_point_sampler="gau_single_sampler", depth_conf_thresh=0.1, geo_cnsst_num=0,
             default_conf=-1, ranges=[-100.0] * 6, alpha_range=0, inall_img=1, n_depth=16, mvs_lr=5e-4, lr=5e-4, verbose=0,
             appr_feature_str0=["imgfeat_0_0123", "dir_0", "point_conf"], appr_feature_str1=["imgfeat_0_0123", "dir_0", "point_conf"],
             appr_feature_str2=["imgfeat_0_0123", "dir_0", "point_conf"], appr_feature_str3=["imgfeat_0_0123", "dir_0", "point_conf"])
    o.update(kw)
    return types.SimpleNamespace(**o)


def _torch_deviation(net, imgs, proj, dv):
    """torch's own device-versus-CPU deviation of the SAME modules, no kernel of this package involved: the float64 restatements of the
    kernels between float32 convolutions on the CPU against the same between the convolutions on `net`'s device -> per-quantity |difference|"""
    import copy
    cpu = copy.deepcopy(net).cpu().float().eval()
    res = []
    with torch.no_grad():
        for m in (cpu, net):
            dev = next(m.parameters()).device
            x = torch.from_numpy(imgs).to(dev)
            feats = torch.stack([m.feature(x[:, v]) for v in range(x.shape[1])], 1).cpu().numpy()
            var = np.concatenate([cost_volume64(feats[b], proj[b:b + 1], dv[b:b + 1], False)[0] for b in range(len(feats))]).astype(np.float32)
            cost = m.cost_regularization(torch.from_numpy(var).to(dev)).squeeze(1).cpu().numpy()
            res.append(regress64(cost, dv))
    return dict(zip(("depth", "idx", "conf", "prob"), (float(np.nanmax(np.abs(a - b))) for a, b in zip(*res))))


def check_e2e(dev):
    """4: MVSNet.forward on the device against its float64 restatement and the reference fixture.  The convolutions between the kernels are
    torch's; where their own device-versus-CPU deviation is the larger one, the bar is four times THAT (printed)."""
    from pointnerf_amd.depth_estimators import MVSNet
    imgs, proj, dv = e2e_inputs()
    net = fill_weights(MVSNet(), E2E["wseed"]).to(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    with torch.no_grad():
        out = net(t(imgs), t(proj), t(dv))
        out_p = net(t(imgs), t(proj), t(dv), prob_only=True)
    assert len(out) == 4 and len(out_p) == 3                                          # the reference's return arity in both forms
    depth, conf, feats, prob = out
    B, V, D = E2E["B"], E2E["V"], E2E["D"]
    h, w = E2E["H"] // 4, E2E["W"] // 4
    assert depth.shape == conf.shape == (B, h, w) and prob.shape == (B, D, h, w) and len(feats) == V and feats[0].shape == (B, 32, h, w)
    assert out_p[1].shape == (B, D, h, w) and out_p[2].shape == (B, D, h, w) and len(out_p[0]) == V
    d64, fi, c64, p64, _ = mvsnet64(net, imgs, proj, dv)
    tdev = _torch_deviation(net, imgs, proj, dv)
    bars = {q: 4 * max(float(fixture()["dev_e2e_" + q]), tdev[q]) for q in tdev}
    print("e2e: torch's own device-vs-CPU deviation", tdev, "reference's fp32 deviation",
          {q: float(fixture()["dev_e2e_" + q]) for q in tdev}, "-> bars", bars)
    ok = decided(fi, bars["idx"])
    assert 1 - ok.mean() <= UNDECIDED_CAP
    depth, conf, prob = (a.cpu().numpy().astype(np.float64) for a in (depth, conf, prob))
    errs = dict(depth=np.abs(depth - d64).max(), conf=np.abs(conf - c64)[ok].max(), prob=np.abs(prob - p64).max(),
                prob_only=np.abs(out_p[1].cpu().numpy() - p64).max())
    print("e2e errors", errs, "median largest probability %.3f" % np.median(p64.max(1)))
    assert errs["depth"] <= bars["depth"] and errs["conf"] <= bars["conf"] and errs["prob"] <= bars["prob"] and errs["prob_only"] <= bars["prob"]
    fx = fixture()
    assert np.abs(depth - fx["e2e_depth"]).max() <= 2 * bars["depth"] and np.abs(prob - fx["e2e_prob"]).max() <= 2 * bars["prob"]
    assert np.abs(conf - fx["e2e_conf"])[ok].max() <= 2 * bars["conf"]
    assert np.median(p64.max(1)) > 0.3                                                # not a flat volume


def check_pyramid(dev):
    import copy
    from pointnerf_amd.depth_estimators import PyramidFeatureNet
    net = fill_weights(PyramidFeatureNet(), PYR["wseed"]).to(dev)
    pim = pyr_inputs()
    with torch.no_grad():
        levels = net(torch.from_numpy(pim).to(dev))
        on_cpu = copy.deepcopy(net).cpu().float()(torch.from_numpy(pim))
    want = pyramid64(net, pim)
    V, H, W = PYR["V"], PYR["H"], PYR["W"]
    assert [tuple(l.shape) for l in levels] == [(V, 3, H, W), (V, 8, H, W), (V, 16, H // 2, W // 2), (V, 32, H // 4, W // 4)]
    assert np.array_equal(levels[0].cpu().numpy(), pim[0])
    tdev = max(float(np.abs(a.cpu().numpy() - b.numpy()).max() / np.abs(w64).max()) for a, b, w64 in zip(levels[1:], on_cpu[1:], want[1:]))
    limit = 4 * max(float(fixture()["dev_pyr"]), tdev)
    for i in (1, 2, 3):
        got = levels[i].cpu().numpy().astype(np.float64)
        err = np.abs(got - want[i]).max() / np.abs(want[i]).max()
        print("pyramid level", i, "err %.3e (bar %.3e; torch device-vs-CPU %.3e)" % (err, limit, tdev))
        assert err <= limit
        assert np.abs(got - fixture()["pyr_level%d" % i]).max() / np.abs(want[i]).max() <= 2 * limit


def check_state_dicts(dev, tmp_path):
    """strict loads with the reference's key lists (names and shapes from the fixture) and load_pretrained_d_est on a checkpoint-shaped file"""
    from pointnerf_amd.depth_estimators import MVSNet, PyramidFeatureNet
    from pointnerf_amd.mvs_points_model import MvsPointsModel
    fx = fixture()
    zeros = lambda keys, shapes: {str(k): torch.zeros([int(s) for s in sh if s >= 0]) for k, sh in zip(keys, shapes)}
    sd = zeros(fx["mvsnet_keys"], fx["mvsnet_shapes"])
    assert "feature.conv0.conv.weight" in sd and "feature.conv0.bn.running_mean" in sd and "cost_regularization.conv7.0.weight" in sd \
        and "cost_regularization.prob.bias" in sd
    MVSNet().load_state_dict(sd, strict=True)
    psd = zeros(fx["pyr_keys"], fx["pyr_shapes"])
    assert "conv0.0.conv.weight" in psd and "conv0.0.bn.running_var" in psd and "toplayer.bias" in psd
    PyramidFeatureNet().load_state_dict(psd, strict=True)
    src = fill_weights(MVSNet(), 31)
    path = str(tmp_path / "model_000014.ckpt")
    torch.save({"model": {"module." + k: v for k, v in src.state_dict().items()}}, path)
    m = MvsPointsModel(make_opt(pre_d_est=path))
    for k, v in src.state_dict().items():
        assert torch.equal(m.MVSNet.state_dict()[k], v), k
    own = set(m.state_dict())
    assert {"FeatureNet." + k for k in psd} | {"MVSNet." + k for k in sd} == own, sorted(own ^ ({"FeatureNet." + k for k in psd} | {"MVSNet." + k for k in sd}))[:5]
    assert not hasattr(MvsPointsModel(make_opt(manual_depth_view=0)), "MVSNet")


# ---- 5. the shell ---------------------------------------------------------------------------------------------------------------------------
SHELL = dict(V=3, H=64, W=96, near_far=(2.5, 7.5), wseed=9, n_depth=16)


def init_item(dev="cpu"):
    """a synthetic ``get_init_item`` dictionary (data/nerf_synth360_ft_dataset.py:479-553, batch dimension in front): three views of the analytic
    sphere-on-a-plane scene of the depth-fusion tests, coloured by the world position each pixel sees"""
    import depthfuse_case as DC
    V, H, W = SHELL["V"], SHELL["H"], SHELL["W"]
    depth, K, E = DC.scene(V, H, W)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    imgs, proj = np.zeros((V, 3, H, W)), np.zeros((V, V, 3, 4))
    P = []
    for v in range(V):
        cam = (pix @ np.linalg.inv(K[v]).T) * depth[v][..., None]
        world = (np.concatenate([cam, np.ones((H, W, 1))], -1) @ np.linalg.inv(E[v]).T)[..., :3]
        for ch in range(3):
            imgs[v, ch] = 0.5 + 0.5 * np.sin(5.0 * world[..., ch] + 3.0 * world[..., (ch + 1) % 3] + ch) * (depth[v] > 0)
        Pl, Kq = np.eye(4), K[v].copy()
        Kq[:2] = Kq[:2] / 4                                                           # :398-400
        Pl[:3, :4] = Kq @ E[v][:3, :4]
        P.append(Pl)
    for i in range(V):                                                                # :506-516
        for j in range(V):
            proj[i, j] = (np.eye(4) if i == j else P[j] @ np.linalg.inv(P[i]))[:3]
    nf = np.asarray(SHELL["near_far"], np.float32)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None].to(dev)
    return dict(images=f32(imgs), mvs_images=f32(imgs), depths_h=f32(depth), alphas=f32(depth > 0), w2cs=f32(E), c2ws=f32(np.linalg.inv(E)),
                near_fars_depth=f32(nf), near_fars=f32(np.tile(nf[None], (V, 1))), proj_mats=f32(proj), intrinsics=f32(K),
                view_ids=torch.arange(V)[None])


def check_shell(dev):
    """create_model(mode=1) -> set_input -> gen_points()'s ten items -> filter_by_masks_gpu -> query_embedding, and the same by hand"""
    from pointnerf_amd import ops, point_init
    from pointnerf_amd.mvs_points_volumetric_model import create_model
    opt = make_opt(n_depth=SHELL["n_depth"], gpu_ids=[int(str(dev).split(":")[1])] if ":" in str(dev) else [])
    model = create_model(opt)
    model.setup(opt)
    model.eval()
    assert model.model_names == ["mvs"] and model.optimizers == [] and not model.net_mvs.training
    fill_weights(model.net_mvs, SHELL["wseed"])
    data = init_item()
    model.set_input(data)
    with torch.no_grad():
        items = model.gen_points()
    assert len(items) == 10
    xyz_lst, conf_lst, mask_lst, K_lst, E_lst, HDWD, c2ws, w2cs, intr, nfs = items
    V, H, W = SHELL["V"], SHELL["H"], SHELL["W"]
    assert len(xyz_lst) == len(conf_lst) == len(mask_lst) == len(K_lst) == len(E_lst) == 2 and tuple(HDWD) == (H, W)
    for x, c, m, k, e in zip(xyz_lst, conf_lst, mask_lst, K_lst, E_lst):
        assert x.shape == (1, 1, 1, H, W, 3) and c.shape == (1, 1, H, W) and m.shape == (1, 1, H, W) and m.dtype == torch.bool
        assert k.shape == (1, 3, 3) and e.shape == (1, 4, 4) and x.is_cuda == c.is_cuda == m.is_cuda
        assert torch.isfinite(x).all() and 0 < int(m.sum())
    assert c2ws.shape == w2cs.shape == (1, V, 4, 4) and intr.shape == (1, V, 3, 3) and nfs.shape == (1, V, 2)
    # by hand: MVSNet.forward on the expanded images, then the tail kernel per view
    net = model.net_mvs.MVSNet
    inp = model.input
    with torch.no_grad():
        depth, conf, _, _ = net(inp["mvs_images"][:, :3].expand(2, -1, -1, -1, -1), inp["proj_mats"][0, :2], point_init.depth_values_of(
            SHELL["near_far"], SHELL["n_depth"]).to(dev).expand(2, -1))
    for i in range(2):
        xyz, cf, mk = ops.depth_to_cam_points(depth[i], conf[i], (H, W), SHELL["near_far"], inp["intrinsics"][0, i])
        err = float((xyz - xyz_lst[i]).abs().max())
        print("shell view", i, "gen_points vs the chain by hand: cam_xyz differs by %.3e, mask by %d pixels" % (err, int((mk != mask_lst[i]).sum())))
        assert err <= 1e-3 and float((mk != mask_lst[i]).float().mean()) <= 0.01      # (torch's convolutions at batch 3 against batch 2 x 1)
    # on into the filter and the embedding
    cam_l, world_l, conf_f = point_init.filter_by_masks_gpu(xyz_lst, K_lst, E_lst, conf_lst, mask_lst, opt)
    assert len(world_l) == 2 and all(len(wl) > 0 for wl in world_l)
    for i in range(2):
        n = len(world_l[i])
        cam_xyz = (torch.cat([world_l[i], torch.ones_like(world_l[i][..., 0:1])], dim=-1) @ E_lst[i][0].t())[..., :3]
        emb, color, dirs, cf = model.query_embedding(HDWD, cam_xyz[None], conf_f[i][None, :, None], inp["images"], c2ws, w2cs, intr, 0, pointdir_w=True)
        assert emb.shape == (1, n, 8 + 16 + 32) and color.shape == (1, n, 3) and dirs.shape == (1, n, 3) and cf.shape == (1, n, 1)
        assert torch.isfinite(emb).all() and float(emb.abs().max()) > 0
    # given depths (manual_depth_view == 0): seven items, no confidence list, the depth map itself behind the clamp
    from pointnerf_amd.mvs_points_model import MvsPointsModel
    m0 = MvsPointsModel(make_opt(manual_depth_view=0)).to(dev)
    out0 = m0.gen_points(dict(inp))
    assert len(out0) == 7 and out0[1] == [] and len(out0[0]) == 2
    d0 = inp["depths_h"][0, 0]
    inside = (d0 >= SHELL["near_far"][0]) & (d0 <= SHELL["near_far"][1])
    assert torch.equal(out0[2][0][0, 0], inside) and float((out0[0][0][0, 0, 0, :, :, 2] - d0)[inside].abs().max()) <= 1e-5
    model.cleanup()
    assert model.net_mvs is None


def check_front_door(dev):
    """points_from_images = depth_maps_from_images followed by points_from_depth_maps; two calls give the same bits"""
    from pointnerf_amd import point_init
    from pointnerf_amd.depth_estimators import MVSNet
    data = init_item(dev)
    net = fill_weights(MVSNet(), SHELL["wseed"]).to(dev)
    imgs, K, E = data["mvs_images"][0], data["intrinsics"][0], data["w2cs"][0]
    views = [[0, 1, 2], [1, 0, 2], [2, 1, 0]]
    args = (net, imgs, K, E, views, SHELL["near_far"])
    depth, conf, mask = point_init.depth_maps_from_images(*args, n_depth=SHELL["n_depth"])
    H, W = SHELL["H"], SHELL["W"]
    assert depth.shape == conf.shape == mask.shape == (3, H, W) and mask.dtype == torch.bool
    assert float(depth.min()) >= SHELL["near_far"][0] - 1e-5 and float(depth.max()) <= SHELL["near_far"][1] + 1e-5
    kw = dict(geo_cnsst_num=0, depth_conf_thresh=0.05)
    a = point_init.points_from_images(*args, n_depth=SHELL["n_depth"], **kw)
    b = point_init.points_from_depth_maps(depth, K, E, conf, mask, **kw)
    assert len(a[0]) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))
    rel = point_init.relative_proj_mats(K, E, [1, 0, 2])
    assert torch.equal(rel[0], torch.eye(4)) and float((rel - torch.cat([data["proj_mats"][0, 1, [1, 0, 2]].cpu(),
                                                                           torch.tensor([0.0, 0, 0, 1]).expand(3, 1, 4)], 1)).abs().max()) <= 1e-4


def check_refusals(dev):
    import pytest
    from pointnerf_amd.depth_estimators import MVSNet
    from pointnerf_amd.mvs_points_model import MvsPointsModel
    from pointnerf_amd.mvs_points_volumetric_model import create_model
    data = init_item(dev)
    for field, value in (("manual_depth_view", -1), ("manual_depth_view", 2), ("manual_std_depth", 0.1), ("far_plane_shift", 0.5)):
        m = MvsPointsModel(make_opt(**{field: value})).to(dev)
        with pytest.raises(NotImplementedError, match=field):
            m.gen_points(dict(data))
    with pytest.raises(NotImplementedError, match="refine"):
        MVSNet(refine=True)
    net = MVSNet().to(dev)
    imgs, proj, dv = (torch.from_numpy(a).to(dev) for a in e2e_inputs())
    with pytest.raises(NotImplementedError, match="gradients"):
        net(imgs, proj, dv)
    net.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="training"):
        net(imgs, proj, dv)
    with pytest.raises(NotImplementedError, match="mode"):
        create_model(make_opt(mode=0))

"""Depth-map fusion (csrc/depthfuse.hip, pointnerf_amd/point_init.py) -- the cases and checks shared by the device suite
(tests/test_gpu_depthfuse.py) and the host emulator (tests/test_depthfuse_emu.py).

Scenes are analytic (a sphere on a plane, exact z-depth per pixel from a ring of cameras), so consistent views really agree.  The fixture
tests/golden/refdepthfuse.npz holds the inputs and what the reference's own source lines compute from them on CPU float32
(tests/golden/make_depthfuse_golden.py); this file restates the filter in float64 numpy (`pairs64`, `hull64`).

The filter's tests are hard thresholds on fp32 arithmetic, so a (pixel, source view) pair is *decided* only when its float64 `dist` and
relative depth difference both lie farther than a margin from their thresholds (1 pixel, 0.01); on decided pairs the verdict must be the
float64 one exactly.  The margins are not tuned to the kernel: they are four times the REFERENCE fixture's own largest fp32 deviation from
the float64 restatement (the factor 4: the kernel folds the intrinsics into the pair matrices and so rounds differently), measured by the
generator over all cases, which also asserts that the reference itself obeys the rule and that at most 1 % of a case's pairs are undecided.
One margin per quantity (dist in pixels, the relative difference, and for the hull the projected pixel and the camera z): each is four
times its own quantity's deviation, which is never looser than one joint margin.  A deviation is measured where it can change a verdict:
on pairs whose float64 dist < 2 and relative difference < 0.02 (a projection that is wrong by 10^3 pixels in float64 and by 10^3 + 1 in
fp32 fails either way), and for the hull on points that project within one pixel of the image."""
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "refdepthfuse.npz")

# measured by tests/golden/make_depthfuse_golden.py on the fixture (reference lines on CPU float32 against float64), then times four:
REF_DEV_DIST, REF_DEV_REL, REF_DEV_AVG = 1.185e-03, 1.853e-05, 1.967e-05      # largest |dist32 - dist64| [pixels], |rel32 - rel64|, |depth_avg32 - 64|
REF_DEV_PX, REF_DEV_Z = 6.109e-06, 1.350e-06                                  # hull: largest |pixel32 - pixel64|, |z32 - z64|
TAU_DIST, TAU_REL, DEPTH_BAR = 4 * REF_DEV_DIST, 4 * REF_DEV_REL, 4 * REF_DEV_AVG
TAU_PX, TAU_Z = 4 * REF_DEV_PX, 4 * REF_DEV_Z
UNDECIDED_CAP = 0.01
E2E_CASE = "v2"                     # the generator's pick: no undecided pair on a kept-or-dropped boundary, none under a kept pixel's average

# name -> (inputs key, geo_cnsst_num, ranges, default_conf)
VARIANTS = {
    "v1": ("v1", 1, None, -1), "v2": ("v2", 1, None, -1),
    "v5_c0": ("v5", 0, None, -1), "v5_c1": ("v5", 1, None, -1), "v5_c3": ("v5", 3, None, -1),
    "v5_ranges": ("v5", 3, [-1.0, -0.6, -0.5, 0.9, 1.2, 1.0], -1), "v5_dc2": ("v5", 3, None, 2),
    "v6": ("v6", 2, None, -1),
}
LIST_CASES = ("v1", "v2", "v5_c0", "v5_c1", "v5_c3", "v5_ranges", "v5_dc2")      # the fixture holds the returned lists of these
CONF_THRESH = 0.1
HULL_COMBOS = [(0, 1), (0, 0), (1, 1), (1, 0)]                  # (with near_far, inall_img)
HULL_NEAR_FAR = (2.5, 5.5)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target):
    """world-to-camera [4,4] float64, z forward, y down"""
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ eye
    return E


def scene(V, H, W, step_deg=14.0, turned=None, focal=None):
    """-> depth [V,H,W], K [V,3,3], E [V,4,4] float64: a sphere (radius 0.7, centre (0, 0, 0.7)) on the plane z = 0 seen from a ring of
    cameras (radius 4, height 2.5); view `turned` looks the other way.  depth = exact camera-z of the first hit, 0 where a ray hits nothing."""
    f = focal if focal is not None else 1.1 * W
    Ks, Es, ds = [], [], []
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(V):
        a = np.deg2rad(step_deg * (v - (V - 1) / 2))
        eye = np.array([4.0 * np.cos(a), 4.0 * np.sin(a), 2.5])
        target = np.array([0.0, 0.0, 0.4])
        if v == turned:
            target = 2 * eye - target
            target[2] = -2.0
        E = look_at(eye, target)
        K = np.array([[f * (1 + 0.01 * v), 0.0, (W - 1) / 2 + 0.3 * v], [0.0, f, (H - 1) / 2 - 0.2 * v], [0.0, 0.0, 1.0]])
        dirs = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K).T              # camera rays with z = 1: t IS the z-depth
        dw = dirs @ E[:3, :3]                                                              # R^T d
        t_plane = np.where(dw[..., 2] < -1e-9, -eye[2] / np.where(dw[..., 2] < -1e-9, dw[..., 2], -1.0), np.inf)
        oc = eye - np.array([0.0, 0.0, 0.7])
        A, B, C = (dw * dw).sum(-1), 2 * (dw @ oc), oc @ oc - 0.49
        disc = B * B - 4 * A * C
        t_sph = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0))) / (2 * A), np.inf)
        t_sph = np.where(t_sph > 0, t_sph, np.inf)
        t = np.minimum(t_plane, t_sph)
        ds.append(np.where(np.isfinite(t), t, 0.0))
        Ks.append(K)
        Es.append(E)
    return np.stack(ds), np.stack(Ks), np.stack(Es)


def make_inputs(key):
    """the fixture's inputs (numpy; float32 where the filter reads them)"""
    rng = np.random.default_rng({"v1": 1, "v2": 2, "v5": 5, "v6": 6}[key])
    if key == "v1":
        d, K, E = scene(1, 7, 5)
    elif key == "v2":
        d, K, E = scene(2, 33, 65)
    elif key == "v6":
        d, K, E = scene(6, 96, 128, step_deg=9.0)
    else:
        d, K, E = scene(5, 33, 65, turned=4)
        d[1] *= 1 + 0.003 * rng.standard_normal(d[1].shape)                                # both tests fire on both sides
        d[2] *= 1 + 0.02 * rng.standard_normal(d[2].shape)
        d[0, 10:18, 20:35] = 0.0                                                           # holes
    V, H, W = d.shape
    conf = np.ones((V, H, W), np.float32)
    pmask = np.ones((V, H, W), bool)
    if key in ("v2", "v5"):
        conf = rng.uniform(0.0, 1.0, (V, H, W)).astype(np.float32)
        pmask = rng.uniform(0.0, 1.0, (V, H, W)) > 0.08
    return dict(depth=d.astype(np.float32), K=K.astype(np.float32), E=E.astype(np.float32), conf=conf, pmask=pmask)


def cam_grid(depth, K):
    """the camera-space grid the filter is given: K^-1 [x y 1] d per pixel (float32 [V,H,W,3]); float64 arithmetic, rounded once"""
    V, H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)
    cam = np.einsum("vij,hwj->vhwi", np.linalg.inv(K.astype(np.float64)), pix) * depth.astype(np.float64)[..., None]
    cam = cam.astype(np.float32)
    cam[..., 2] = depth                                                                    # the depth map itself, bit for bit
    return cam


def make_hull_inputs():
    rng = np.random.default_rng(11)
    d, K, E = scene(4, 33, 65, step_deg=25.0)
    yy, xx = np.mgrid[0:33, 0:65]
    ell = np.stack([(xx - 32 - 2 * v) ** 2 / 600.0 + (yy - 16) ** 2 / 150.0 for v in range(4)])
    alphas = np.where(ell < 1, 1.0, np.where(ell < 1.3, 0.08, 0.0)).astype(np.float32)     # foreground, a rim below the 0.1 bar, background
    pts = np.concatenate([rng.uniform(-0.9, 0.9, (1800, 3)) + [0, 0, 0.6],                 # inside / around the silhouettes
                          rng.uniform(-4.0, 4.0, (800, 3)),                                # outside the images
                          rng.uniform(-1.0, 1.0, (400, 3)) * [3.0, 3.0, 0.5] + [9.0, 0.0, 2.5]])   # behind the cameras
    return dict(points=pts.astype(np.float32), alphas=alphas, K=K.astype(np.float32), E=E.astype(np.float32))


# ---- float64 restatements ----------------------------------------------------------------------------------------------------------------
def _bilinear_border64(img, x, y):
    H, W = img.shape
    xc, yc = np.clip(np.nan_to_num(x, nan=0.0, posinf=W - 1, neginf=0.0), 0, W - 1), np.clip(np.nan_to_num(y, nan=0.0, posinf=H - 1, neginf=0.0), 0, H - 1)
    x0, y0 = np.floor(xc).astype(np.int64), np.floor(yc).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = xc - x0, yc - y0
    return (img[y0, x0] * (1 - wx) * (1 - wy) + img[y0, x1] * wx * (1 - wy) + img[y1, x0] * (1 - wx) * wy + img[y1, x1] * wx * wy)


def pairs64(depth, K, E):
    """filter_utils.py:157-215 in float64 on the float32 inputs -> dist, rel, d_rep [V,V,H,W] (the diagonal is NaN)"""
    depth, K, E = depth.astype(np.float64), K.astype(np.float64), E.astype(np.float64)
    V, H, W = depth.shape
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
    dist, rel, drep = (np.full((V, V, H, W), np.nan) for _ in range(3))
    with np.errstate(all="ignore"):
        for r in range(V):
            xyz_ref = np.linalg.inv(K[r]) @ (pix * depth[r].ravel())
            for s in range(V):
                if s == r:
                    continue
                xyz_src = (E[s] @ np.linalg.inv(E[r]) @ np.vstack([xyz_ref, np.ones(H * W)]))[:3]
                kx = K[s] @ xyz_src
                xy_src = kx[:2] / kx[2:3]
                d_s = _bilinear_border64(depth[s], xy_src[0], xy_src[1])
                xyz_s = np.linalg.inv(K[s]) @ (np.vstack([xy_src, np.ones(H * W)]) * d_s)
                xyz_rep = (E[r] @ np.linalg.inv(E[s]) @ np.vstack([xyz_s, np.ones(H * W)]))[:3]
                kr = K[r] @ xyz_rep
                xy_rep = kr[:2] / kr[2:3]
                dist[r, s] = np.sqrt((xy_rep[0] - pix[0]) ** 2 + (xy_rep[1] - pix[1]) ** 2).reshape(H, W)
                rel[r, s] = (np.abs(xyz_rep[2] - depth[r].ravel()) / depth[r].ravel()).reshape(H, W)
                drep[r, s] = xyz_rep[2].reshape(H, W)
    return dist, rel, drep


def verdicts64(depth, K, E, tau_dist=None, tau_rel=None):
    """-> dict: passing [V,V,H,W] bool (float64 verdict), decided [V,V,H,W] bool, geo [V,H,W], avg [V,H,W] float64, all_decided [V,H,W],
    undecided_fraction (of the V (V - 1) H W pairs)"""
    tau_dist = TAU_DIST if tau_dist is None else tau_dist
    tau_rel = TAU_REL if tau_rel is None else tau_rel
    dist, rel, drep = pairs64(depth, K, E)
    V = depth.shape[0]
    with np.errstate(all="ignore"):
        passing = (dist < 1) & (rel < 0.01)
        undecided = (np.abs(dist - 1) <= tau_dist) | (np.abs(rel - 0.01) <= tau_rel)      # NaN / inf: decided, fails
    off = ~np.eye(V, dtype=bool)[:, :, None, None]
    passing, undecided = passing & off, undecided & off
    geo = passing.sum(1)
    avg = (np.where(passing, drep, 0.0).sum(1) + depth.astype(np.float64)) / (geo + 1)
    n_pairs = max(V * (V - 1) * depth.shape[1] * depth.shape[2], 1)
    return dict(dist=dist, rel=rel, passing=passing, decided=~undecided, geo=geo, avg=avg, all_decided=~undecided.any(1),
                undecided_fraction=undecided.sum() / n_pairs)


def hull64(points, alphas, K, E, near_far, use_range):
    """mvs_utils.py:573-607 in float64 -> mask [N] bool, px [V,N,2], z [V,N]"""
    p = np.concatenate([points.astype(np.float64), np.ones((len(points), 1))], -1)
    V, H, W = alphas.shape
    keep = np.ones(len(points), bool)
    pxs, zs = [], []
    with np.errstate(all="ignore"):
        for v in range(V):
            cam = p @ E[v].astype(np.float64).T
            q = cam[:, :3] @ K[v].astype(np.float64).T
            px = q[:, :2] / q[:, 2:3]
            f = np.floor(px)
            inside = (f[:, 0] >= 0) & (f[:, 0] < W) & (f[:, 1] >= 0) & (f[:, 1] < H)
            ix = np.clip(np.nan_to_num(f[:, 0]), 0, W - 1).astype(np.int64)
            iy = np.clip(np.nan_to_num(f[:, 1]), 0, H - 1).astype(np.int64)
            m = alphas[v][iy, ix].astype(np.float64)
            if use_range:
                m = m + (~inside)
            ok = m > 0.1
            if near_far is not None:
                ok &= (cam[:, 2] >= near_far[0] - 1.0) & (cam[:, 2] <= near_far[1])
            keep &= ok
            pxs.append(px)
            zs.append(cam[:, 2])
    return keep, np.stack(pxs), np.stack(zs)


def hull_decided(px, z, H, W, near_far, tau_px=None, tau_z=None):
    """points farther than tau_px from every integer pixel boundary that can matter (0 .. W, 0 .. H: beyond them the clamp decides) in
    every view and, with near_far, farther than tau_z from its bounds"""
    tau_px = TAU_PX if tau_px is None else tau_px
    tau_z = TAU_Z if tau_z is None else tau_z
    with np.errstate(all="ignore"):
        def near_boundary(c, n):
            cc = np.nan_to_num(c, nan=-1e9, posinf=1e9, neginf=-1e9)
            return (cc > -0.5) & (cc < n + 0.5) & (np.abs(cc - np.round(cc)) <= tau_px)
        und = near_boundary(px[..., 0], W) | near_boundary(px[..., 1], H)
        if near_far is not None:
            und |= (np.abs(z - (near_far[0] - 1.0)) <= tau_z) | (np.abs(z - near_far[1]) <= tau_z)
    return ~und.any(0)


# ---- the fixture and the product ------------------------------------------------------------------------------------------------------------
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with np.load(FIX) as z:
            _fx = {k: z[k] for k in z.files}
    return _fx


def inputs(key):
    fx = fixture()
    out = {k: fx["%s_%s" % (key, k)] for k in ("depth", "K", "E")}
    V, H, W = out["depth"].shape
    out["conf"] = fx["%s_conf" % key] if "%s_conf" % key in fx else np.ones((V, H, W), np.float32)
    out["pmask"] = fx["%s_pmask" % key].astype(bool) if "%s_pmask" % key in fx else np.ones((V, H, W), bool)
    return out


def make_opt(name):
    _, cnsst, ranges, dconf = VARIANTS[name]
    return types.SimpleNamespace(manual_depth_view=1, depth_conf_thresh=CONF_THRESH, geo_cnsst_num=cnsst, default_conf=dconf,
                                 far_plane_shift=None, ranges=ranges if ranges is not None else [-100.0] * 6, alpha_range=0, inall_img=1)


def list_args(inp, dev="cpu"):
    """the reference's list-of-tensors arguments"""
    cam = cam_grid(inp["depth"], inp["K"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    V = cam.shape[0]
    return ([t(cam[v])[None, None, None] for v in range(V)], [t(inp["K"][v])[None] for v in range(V)], [t(inp["E"][v])[None] for v in range(V)],
            [t(inp["conf"][v])[None, None] for v in range(V)], [t(inp["pmask"][v])[None, None] for v in range(V)])


_dense = {}


def dense(key, dev):
    """the kernel's dense maps of one input set (computed once per device) and their float64 verdicts"""
    if (key, dev) not in _dense:
        from pointnerf_amd import point_init
        inp = inputs(key)
        t = lambda a: torch.from_numpy(a).to(dev)
        geo, avg = point_init.depth_consistency(t(inp["depth"]), t(inp["K"]), t(inp["E"]))
        assert geo.dtype == torch.int32 and avg.dtype == torch.float32 and geo.shape == avg.shape == inp["depth"].shape
        _dense[(key, dev)] = (geo.cpu().numpy(), avg.cpu().numpy(), verdicts64(inp["depth"], inp["K"], inp["E"]))
    return _dense[(key, dev)]


# ---- checks ----------------------------------------------------------------------------------------------------------------------------
def check_thresholds(key, dev):
    """1 + 2: geo_mask_sum equals the float64 verdict and the fixture's count on pixels all of whose pairs are decided; depth_avg within
    DEPTH_BAR of float64 there"""
    assert TAU_DIST > 0 and TAU_REL > 0 and DEPTH_BAR > 0, "margins not recorded"
    geo, avg, v64 = dense(key, dev)
    fx = fixture()
    print(key, "undecided pairs %.4f %%" % (100 * v64["undecided_fraction"]), "pixels checked %d of %d" % (v64["all_decided"].sum(), geo.size))
    assert v64["undecided_fraction"] <= UNDECIDED_CAP
    ok = v64["all_decided"]
    assert ok.sum() >= 0.9 * ok.size
    assert np.array_equal(geo[ok], v64["geo"][ok]), "%d decided pixels differ from float64" % (geo[ok] != v64["geo"][ok]).sum()
    assert np.array_equal(geo[ok], fx["%s_geo" % key].astype(np.int32)[ok])
    with np.errstate(all="ignore"):
        err = np.abs(avg.astype(np.float64) - v64["avg"])[ok]
    err = err[np.isfinite(v64["avg"][ok])]
    print(key, "depth_avg max err %.3e (bar %.3e)" % (err.max(), DEPTH_BAR))
    assert err.max() <= DEPTH_BAR
    if geo.shape[0] == 1:
        inp = inputs(key)
        assert not geo.any() and np.array_equal(avg, inp["depth"])


def restate_select(geo, avg, inp, opt):
    """filter_utils.py:259-291 in torch (CPU float32) on given dense maps -> the three lists"""
    cam = torch.from_numpy(cam_grid(inp["depth"], inp["K"]))
    geo, avg = torch.from_numpy(geo), torch.from_numpy(avg)
    conf_all, pm_all, E = torch.from_numpy(inp["conf"]), torch.from_numpy(inp["pmask"]), torch.from_numpy(inp["E"])
    V = cam.shape[0]
    out = ([], [], [])
    for v in range(V):
        confidence = conf_all[v]
        final_mask = torch.logical_and(confidence > opt.depth_conf_thresh, pm_all[v])
        final_mask = torch.logical_and(final_mask, geo[v] >= opt.geo_cnsst_num) if V > 1 else final_mask
        xy, depth = cam[v][..., :-1][final_mask, :], avg[v][final_mask][..., None]
        xyz_cam = torch.cat([xy, depth], dim=-1)
        cf = confidence[final_mask]
        if opt.default_conf > 1.0:
            g = geo[v][final_mask] - opt.geo_cnsst_num + 1
            cf = cf * (1 - 1.0 / torch.pow(1.14869, torch.clamp(g, min=1, max=10)))
        xyz_world = torch.cat([xyz_cam, torch.ones_like(xyz_cam[..., 0:1])], axis=-1) @ torch.inverse(E[v]).transpose(0, 1)
        if opt.ranges[0] > -99.0:
            ranges = torch.as_tensor(opt.ranges, dtype=torch.float32)
            m = torch.prod(torch.logical_and(xyz_world[..., :3] >= ranges[None, :3], xyz_world[..., :3] <= ranges[None, 3:]), dim=-1) > 0
            xyz_world, xyz_cam, cf = xyz_world[m], xyz_cam[m], cf[m]
        out[0].append(xyz_cam)
        out[1].append(xyz_world[:, :3])
        out[2].append(cf)
    return out


def run_filter(name, dev):
    from pointnerf_amd import point_init
    inp = inputs(VARIANTS[name][0])
    return point_init.filter_by_masks_gpu(*list_args(inp, dev), make_opt(name)), inp


def check_selection(name, dev):
    """3: lists of exactly the restatement's lengths and order; xyz_cam and confidence bit-equal, xyz_world within 4 ulp of its largest
    coordinate.  A world position within that rounding of a `ranges` face may be kept by one and dropped by the other: none occurs on
    these inputs (the lengths are compared exactly)."""
    (cam_l, world_l, conf_l), inp = run_filter(name, dev)
    geo, avg, _ = dense(VARIANTS[name][0], dev)
    r_cam, r_world, r_conf = restate_select(geo, avg, inp, make_opt(name))
    V = inp["depth"].shape[0]
    assert len(cam_l) == len(world_l) == len(conf_l) == V
    kept = 0
    for v in range(V):
        assert cam_l[v].shape == r_cam[v].shape and world_l[v].shape == r_world[v].shape and conf_l[v].shape == r_conf[v].shape, (name, v)
        assert torch.equal(cam_l[v].cpu(), r_cam[v]) and torch.equal(conf_l[v].cpu(), r_conf[v]), (name, v)
        if len(r_world[v]):
            big = float(r_world[v].abs().max())
            ulp = float(np.spacing(np.float32(big)))
            err = float((world_l[v].cpu() - r_world[v]).abs().max())
            assert err <= 4 * ulp, (name, v, err, ulp)
        kept += len(r_cam[v])
    print(name, "kept", kept)
    if V == 1:                                   # no geometric clause: geo_mask_sum is all zero and geo_cnsst_num = 1, yet pixels are kept
        assert kept == int(((inp["conf"] > CONF_THRESH) & inp["pmask"]).sum()) > 0
    else:
        assert 0 < kept < inp["depth"].size
    return kept


def check_fixture_end_to_end(dev, name=E2E_CASE):
    """4: the three returned lists against the reference's, in length, order and value"""
    (cam_l, world_l, conf_l), inp = run_filter(name, dev)
    fx = fixture()
    sizes = fx["%s_sizes" % name]
    assert [len(c) for c in cam_l] == sizes.tolist()
    for got, key in ((cam_l, "xyz_cam"), (world_l, "xyz_world"), (conf_l, "conf")):
        g = torch.cat(got).cpu().numpy().astype(np.float64)
        err = np.abs(g - fx["%s_out_%s" % (name, key)].astype(np.float64)).max()
        print(name, key, "max err %.3e" % err)
        assert err <= DEPTH_BAR


def check_hull(dev):
    """5"""
    from pointnerf_amd import point_init
    assert TAU_PX > 0 and TAU_Z > 0, "margins not recorded"
    fx = fixture()
    pts, alphas, K, E = fx["hull_points"], fx["hull_alphas"], fx["hull_K"], fx["hull_E"]
    V, H, W = alphas.shape
    t = lambda a: torch.from_numpy(a).to(dev)
    for i, (with_nf, inall) in enumerate(HULL_COMBOS):
        nf = HULL_NEAR_FAR if with_nf else None
        opt = types.SimpleNamespace(alpha_range=0, inall_img=inall)
        got = point_init.alpha_masking(t(pts), [alphas[v][None] for v in range(V)], [K[v] for v in range(V)], None, [E[v] for v in range(V)], nf, opt=opt)
        assert got.dtype == torch.bool and got.shape == (len(pts),)
        got = got.cpu().numpy()
        want, px, z = hull64(pts, alphas, K, E, nf, inall == 0)
        ok = hull_decided(px, z, H, W, nf)
        print("hull", with_nf, inall, "kept %d, undecided %d" % (want.sum(), (~ok).sum()))
        assert (~ok).mean() <= UNDECIDED_CAP
        assert np.array_equal(got[ok], want[ok]), (with_nf, inall, int((got[ok] != want[ok]).sum()))
        assert np.array_equal(got[ok], fx["hull_mask_%d" % i].astype(bool)[ok])
        assert 0 < want.sum() < len(pts)


def check_refusals(dev):
    """6"""
    import ctypes
    import pytest
    from pointnerf_amd import point_init, _lib as L
    inp = inputs("v2")
    args = list_args(inp, dev)
    for field, value, word in (("manual_depth_view", 2, "manual_depth_view"), ("far_plane_shift", 0.1, "far_plane_shift")):
        opt = make_opt("v2")
        setattr(opt, field, value)
        with pytest.raises(NotImplementedError, match=word):
            point_init.filter_by_masks_gpu(*args, opt)
    # views of unequal size
    bad = [a.clone() for a in args[0]]
    bad[1] = bad[1][:, :, :, :-1].contiguous()
    with pytest.raises(RuntimeError, match="PNERF_E_UNSUP"):
        point_init.filter_by_masks_gpu(bad, *args[1:], make_opt("v2"))
    t = lambda a: torch.from_numpy(a).to(dev)
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):                       # H = 1
        point_init.depth_consistency(t(inp["depth"][:, :1].copy()), t(inp["K"]), t(inp["E"]))
    # the C ABI itself
    lib = L.lib()
    V, H, W = inp["depth"].shape
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(t(inp["depth"]).data_ptr())                              # a valid pointer: nothing is launched on a refusal
    hw = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.pnerf_depth_consistency(one, hw(H, W, H, W), 2, one, z, one, z) == -1          # null output
    assert lib.pnerf_depth_consistency(one, hw(H, W, H, W + 1), 2, one, one, one, z) == -4    # views of different size
    assert lib.pnerf_depth_consistency(one, hw(1, W, 1, W), 2, one, one, one, z) == -1        # H < 2
    assert lib.pnerf_depth_consistency(one, hw(H, W), 0, one, one, one, z) == -1              # V < 1
    assert lib.pnerf_depth_fuse_select_workspace_bytes(0, H, W) == 0 and lib.pnerf_depth_fuse_select_workspace_bytes(2, 1, W) == 0
    nws = lib.pnerf_depth_fuse_select_workspace_bytes(V, H, W)
    assert nws > 8 * V * H * W
    sel = lambda xyz_cam, ws_bytes, h=H: lib.pnerf_depth_fuse_select(one, one, one, one, one, one, V, h, W, 0.1, 1, None, None, xyz_cam, one, one, one, one,
                                                                  one, ws_bytes, z)
    assert sel(z, nws) == -1 and sel(one, nws - 1) == -2 and sel(one, nws, 1) == -1
    assert lib.pnerf_alpha_hull(one, 10, one, one, one, 2, H, W, 0, None, z, z) == -1
    assert lib.pnerf_alpha_hull(one, 10, one, one, one, 0, H, W, 0, None, one, z) == -1
    assert lib.pnerf_alpha_hull(z, 0, z, z, z, 2, H, W, 0, None, z, z) == 0


def check_cpu_tensors_refused():
    """the device path has no CPU implementation"""
    import pytest
    from pointnerf_amd import point_init
    inp = inputs("v2")
    t = torch.from_numpy
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.filter_by_masks_gpu(*list_args(inp, "cpu"), make_opt("v2"))
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.depth_consistency(t(inp["depth"]), t(inp["K"]), t(inp["E"]))
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.alpha_masking(torch.zeros(4, 3), [np.ones((1, 4, 4), np.float32)], [np.eye(3)], None, [np.eye(4)], None)
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.points_from_depth_maps(t(inp["depth"]), t(inp["K"]), t(inp["E"]), geo_cnsst_num=1, depth_conf_thresh=0.1)


def front_alphas(inp):
    """the carving views keep a central window; the view that looks away sees every candidate outside its image, at the clamped border"""
    al = np.zeros(inp["depth"].shape, np.float32)
    al[:, 4:30, 12:50] = 1.0
    al[4] = 1.0
    return al


def front_door(dev, vox_res=0):
    from pointnerf_amd import point_init
    inp = inputs("v5")
    t = lambda a: torch.from_numpy(a).to(dev)
    alphas = t(front_alphas(inp))
    return point_init.points_from_depth_maps(t(inp["depth"]), t(inp["K"]), t(inp["E"]), t(inp["conf"]), t(inp["pmask"]), alphas, geo_cnsst_num=1,
                                             depth_conf_thresh=CONF_THRESH, vox_res=vox_res)


def check_reproducible(dev):
    """7a: two calls, the same bits; the front door = filter + hull"""
    from pointnerf_amd import point_init
    a, _ = run_filter("v5_dc2", dev)
    b, _ = run_filter("v5_dc2", dev)
    for la, lb in zip(a, b):
        assert all(torch.equal(x, y) for x, y in zip(la, lb))
    inp = inputs("v5")
    t = lambda x: torch.from_numpy(x).to(dev)
    g1 = point_init.depth_consistency(t(inp["depth"]), t(inp["K"]), t(inp["E"]))
    g2 = point_init.depth_consistency(t(inp["depth"]), t(inp["K"]), t(inp["E"]))
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    xyz, cf, vid = front_door(dev)
    xyz2, cf2, vid2 = front_door(dev)
    assert torch.equal(xyz, xyz2) and torch.equal(cf, cf2) and torch.equal(vid, vid2)
    # the same points as the list interface followed by alpha_masking
    (_, world_l, conf_l), _ = run_filter("v5_c1", dev)
    world, conf = torch.cat(world_l), torch.cat(conf_l)
    ids = torch.cat([torch.full((len(w),), v, dtype=torch.int64) for v, w in enumerate(world_l)]).to(world.device)
    V = inp["depth"].shape[0]
    al = front_alphas(inp)
    keep = point_init.alpha_masking(world, [al[v][None] for v in range(V)], [inp["K"][v] for v in range(V)], None, [inp["E"][v] for v in range(V)], None)
    assert 0 < int(keep.sum()) < len(keep)
    # (the front door back-projects with its own K^-1: x, y of xyz_cam do not enter xyz_world's z-driven part identically, so compare loosely)
    assert len(xyz) == int(keep.sum()) and torch.equal(vid, ids[keep]) and torch.equal(cf, conf[keep])
    assert float((xyz - world[keep]).abs().max()) <= 1e-5


def check_vox_chain(dev):
    """7b: vox_res = 24 returns what construct_vox_points_closest returns on the unvoxelised result, with the gathered confidence and ids"""
    from pointnerf_amd import point_init
    xyz, cf, vid = front_door(dev)
    vx, vc, vv = front_door(dev, vox_res=24)
    cen, _, idx = point_init.construct_vox_points_closest(xyz, 24)
    assert 0 < len(cen) < len(xyz)
    assert torch.equal(vx, cen) and torch.equal(vc, cf[idx]) and torch.equal(vv, vid[idx])

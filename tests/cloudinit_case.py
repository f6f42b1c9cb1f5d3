"""Points from an external cloud (csrc/cloudinit.hip, pointnerf_amd/point_init.py) -- the cases and checks shared by the device suite
(tests/test_gpu_cloudinit.py) and the host emulator (tests/test_cloudinit_emu.py).

The fixture tests/golden/refcloudinit.npz holds the inputs and what the reference's own source lines compute from them on CPU float32
(tests/golden/make_cloudinit_golden.py: nearest_view, construct_vox_points_ind, the occupancy merge, the crop, the split into views).

Merge, crop and grouping are exact.  The nearest view is an argmin over fp32 scores, so it is held to the float64 restatement `score64`
where that can be asked: a point is *decided* when its float64 runner-up exceeds its float64 best by more than 2 TAU; there the index must
be the float64 argmin, elsewhere the float64 score of the chosen camera must lie within 2 TAU of the best.  TAU is not tuned to the kernel:
it is four times REF_DEV, the largest |score32 - score64| of the REFERENCE's lines over all cases (the factor 4: the kernel divides the dot
product once where the reference divides three components, so it rounds differently), measured by the generator, which also asserts that
the reference itself obeys the rule and that at most 1 % of a case's points are undecided.  In the case with two bit-identical cameras
(3 and 17) the copy's column is left out of the analysis: its score equals camera 3's in any arithmetic, so no minimum changes, and the
result must never be 17 (ties go to the lowest index)."""
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "refcloudinit.npz")

# measured by tests/golden/make_cloudinit_golden.py (reference lines on CPU float32 against float64 over all cases), then times four:
REF_DEV = 2.897e-07
TAU = 4 * REF_DEV
UNDECIDED_CAP = 0.01
E2E_CASE = "e2e_a"                  # the generator's pick: no undecided point among the points that reach nearest_view

LDS_CHUNK = 256                     # NV_CHUNK of csrc/cloudinit.hip: camera records per LDS stage
# name -> (N, M, cameras, half width of the points' cube, scale, twin)
NV_CASES = {
    "m1": (257, 1, "ring", 1.2, 1.0, None),
    "ring24": (5000, 24, "ring", 1.2, 1.0, None),
    "chunk": (513, 2 * LDS_CHUNK + 37, "shell", 3.0, 1.0, None),
    "ring24_x30": (5000, 24, "ring", 1.2, 30.0, None),
    "twin": (1000, 24, "ring", 1.2, 1.0, (3, 17)),
    "empty": (0, 24, "ring", 1.2, 1.0, None),
}
MERGE_RES = (100, 7)
CROP_RANGES = {"box": [-0.8, -1.5, -0.3, 1.1, 0.9, 1.6], "nothing": [5.0, 5.0, 5.0, 6.0, 6.0, 6.0]}
E2E_CANDIDATES = ("e2e_a", "e2e_b", "e2e_c", "e2e_d", "e2e_e", "e2e_f", "e2e_g", "e2e_h")
E2E_RANGES = [-1.5, -1.4, -1.2, 1.5, 1.5, 1.3]
E2E_MERGE_RES = 100
# name -> (N, M, views drawn from)
GROUP_CASES = {"one": (1, 5, [3]), "blocks": (70000, 300, list(range(2, 300, 3))), "single_view": (3000, 7, [4]), "few": (1500, 2, [0, 1]),
               "empty": (0, 4, [0])}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def cameras(kind, M, seed=0):
    """-> campos [M,3], camdir [M,3] float32.  "ring": M cameras on a circle of radius 4 at height 1.5 looking at the origin; "shell":
    cameras spread over a sphere (radii 5 .. 7) looking at jittered targets near the origin"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "ring":
        a = 2 * np.pi * np.arange(M) / max(M, 1)
        pos = np.stack([4 * np.cos(a), 4 * np.sin(a), np.full(M, 1.5)], -1)
        target = np.zeros((M, 3))
    else:
        k = np.arange(M) + 0.5
        phi, th = np.arccos(1 - 2 * k / M), np.pi * (1 + 5 ** 0.5) * k
        rad = rng.uniform(5.0, 7.0, M)
        pos = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], -1) * rad[:, None]
        target = rng.uniform(-0.5, 0.5, (M, 3))
    d = target - pos
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return pos.astype(np.float32), d.astype(np.float32)


def make_nv_inputs(name):
    N, M, kind, half, scale, twin = NV_CASES[name]
    rng = np.random.default_rng(list(NV_CASES).index(name) + 1)
    campos, camdir = cameras(kind, M)
    xyz = rng.uniform(-half, half, (N, 3)).astype(np.float32)
    if scale != 1.0:
        xyz, campos = xyz * np.float32(scale), campos * np.float32(scale)
    if twin is not None:
        campos[twin[1]], camdir[twin[1]] = campos[twin[0]], camdir[twin[0]]
    return dict(xyz=xyz, campos=campos, camdir=camdir)


def make_merge_inputs():
    rng = np.random.default_rng(21)
    return dict(a=rng.uniform(-1.0, 1.0, (4000, 3)).astype(np.float32), b=rng.uniform(-1.6, 1.6, (3000, 3)).astype(np.float32))


def make_e2e_inputs(name):
    """a small cloud, a second cloud that partly repeats it (so the merge removes something), the 24-camera ring with three cameras
    turned away (they win no point)"""
    rng = np.random.default_rng(40 + E2E_CANDIDATES.index(name))
    a = rng.uniform(-1.2, 1.2, (150, 3))
    b = np.concatenate([a[:50] + rng.uniform(-2e-3, 2e-3, (50, 3)), rng.uniform(-1.7, 1.7, (70, 3))])
    campos, camdir = cameras("ring", 24)
    camdir[[5, 6, 20]] *= -1
    return dict(a=a.astype(np.float32), b=b[rng.permutation(len(b))].astype(np.float32), campos=campos, camdir=camdir)


def make_group_input(name):
    N, M, views = GROUP_CASES[name]
    rng = np.random.default_rng(60 + list(GROUP_CASES).index(name))
    return np.asarray(views, np.int64)[rng.integers(0, len(views), N)], M


# ---- float64 restatement -------------------------------------------------------------------------------------------------------------------
def score64(xyz, campos, camdir):
    """run/train_ft.py:43-46 in float64 on the float32 inputs -> [N,M]"""
    d = xyz.astype(np.float64)[:, None, :] - campos.astype(np.float64)[None]
    nrm = np.sqrt((d * d).sum(-1))
    return nrm / 200 + (1.1 - ((d / (nrm[..., None] + 1e-6)) * camdir.astype(np.float64)[None]).sum(-1))


def verdict64(s64, twin=None, tau=None):
    """-> best [N], arg [N], decided [N] of the float64 scores (the twin's copy left out)"""
    tau = TAU if tau is None else tau
    s = s64.copy()
    if twin is not None:
        s[:, twin[1]] = np.inf
    N, M = s.shape
    arg = s.argmin(1) if N else np.zeros(0, np.int64)
    best = s[np.arange(N), arg]
    if M > 1 and N:
        runner = np.partition(s, 1, axis=1)[:, 1]
    else:
        runner = np.full(N, np.inf)
    return best, arg, (runner - best) > 2 * tau


def obeys_rule(got, s64, twin=None, tau=None):
    """-> (ok, undecided fraction, message)"""
    tau = TAU if tau is None else tau
    best, arg, decided = verdict64(s64, twin, tau)
    N = len(best)
    if N == 0:
        return len(got) == 0, 0.0, "empty"
    wrong = int((got[decided] != arg[decided]).sum())
    slack = s64[np.arange(N), got] - best
    far = int((slack[~decided] > 2 * tau).sum())
    und = float((~decided).mean())
    return wrong == 0 and far == 0, und, "%d decided points differ from float64, %d undecided ones lie beyond 2 TAU; undecided %.3f %%" % (wrong, far, 100 * und)


# ---- the fixture and the product -------------------------------------------------------------------------------------------------------------
_fx = None


def fixture():
    global _fx
    if _fx is None:
        with np.load(FIX) as z:
            _fx = {k: z[k] for k in z.files}
    return _fx


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_ran = {}


def run_nearest(name, dev):
    """the product's nearest_view on one case (computed once per device)"""
    if (name, dev) not in _ran:
        from pointnerf_amd import point_init
        inp = make_nv_inputs(name)
        got = point_init.nearest_view(_t(inp["campos"], dev), _t(inp["camdir"], dev), _t(inp["xyz"], dev), None)
        assert got.dtype == torch.int64 and tuple(got.shape) == (len(inp["xyz"]), 1), (got.dtype, got.shape)
        _ran[(name, dev)] = (inp, got.cpu().numpy()[:, 0])
    return _ran[(name, dev)]


# ---- checks ------------------------------------------------------------------------------------------------------------------------------------
def check_nearest(name, dev):
    """the accuracy rule against float64, the fixture's index on decided points, the generated inputs are the fixture's"""
    assert TAU > 0, "margin not recorded"
    inp, got = run_nearest(name, dev)
    fx = fixture()
    twin = NV_CASES[name][5]
    assert np.array_equal(inp["xyz"], fx["nv_%s_xyz" % name]) and np.array_equal(inp["campos"], fx["nv_%s_campos" % name])
    assert np.array_equal(inp["camdir"], fx["nv_%s_camdir" % name])
    N, M = len(inp["xyz"]), len(inp["campos"])
    assert got.shape == (N,) and (N == 0 or (got.min() >= 0 and got.max() < M))
    s64 = score64(inp["xyz"], inp["campos"], inp["camdir"])
    ok, und, msg = obeys_rule(got, s64, twin)
    print(name, msg)
    assert ok, msg
    assert und <= UNDECIDED_CAP, und
    _, _, decided = verdict64(s64, twin)
    assert np.array_equal(got[decided], fx["nv_%s_cam_ind" % name][decided])
    if twin is not None:
        assert not (got == twin[1]).any() and (got == twin[0]).any()
    if M > 1 and N:
        assert len(np.unique(got)) > 1


def merge_space(a, res):
    """mvs_utils.py:524-531 in torch float32 on the CPU -> what the host passes"""
    a = torch.from_numpy(a)
    xyz_min, xyz_max = torch.min(a, dim=-2)[0], torch.max(a, dim=-2)[0]
    space_edge = torch.max(xyz_max - xyz_min) * 1.05
    xyz_mid = (xyz_max + xyz_min) / 2
    return xyz_mid - space_edge / 2, xyz_mid + space_edge / 2


def check_merge(dev):
    """the kept mask and rows equal the fixture's at both resolutions; A == B keeps nothing; an empty B; an empty A keeps everything"""
    from pointnerf_amd import point_init
    fx = fixture()
    a, b = fx["merge_a"], fx["merge_b"]
    m = make_merge_inputs()
    assert np.array_equal(a, m["a"]) and np.array_equal(b, m["b"])
    for res in MERGE_RES:
        kept, mask = point_init.merge_by_occupancy(_t(a, dev), _t(b, dev), res, return_mask=True)
        assert mask.dtype == torch.bool and kept.dtype == torch.float32
        want = fx["merge_mask_%d" % res].astype(bool)
        print("merge res %d: kept %d of %d" % (res, want.sum(), len(want)))
        assert np.array_equal(mask.cpu().numpy(), want), int((mask.cpu().numpy() != want).sum())
        assert np.array_equal(kept.cpu().numpy(), b[want])
        assert 0 < want.sum() < len(want)
        only = point_init.merge_by_occupancy(_t(a, dev), _t(b, dev), res)
        assert torch.equal(only, kept)
    # most of B lies outside A's cube and is kept for that
    smin, smax = merge_space(a, 100)
    outside = ((torch.from_numpy(b) < smin) | (torch.from_numpy(b) > smax)).any(-1).numpy()
    assert outside.mean() > 0.5 and fx["merge_mask_7"].astype(bool)[outside].all()
    for res in MERGE_RES:
        kept, mask = point_init.merge_by_occupancy(_t(a, dev), _t(a, dev), res, return_mask=True)
        assert len(kept) == 0 and not mask.any()
        kept, mask = point_init.merge_by_occupancy(_t(a, dev), _t(b[:0], dev), res, return_mask=True)
        assert tuple(kept.shape) == (0, 3) and tuple(mask.shape) == (0,)
        kept = point_init.merge_by_occupancy(_t(a[:0], dev), _t(b, dev), res)
        assert np.array_equal(kept.cpu().numpy(), b)


def check_crop(dev):
    """the crop equals torch's boolean indexing (run/train_ft.py:675-680 restated), and the fixture's"""
    from pointnerf_amd import point_init
    fx = fixture()
    b = fx["merge_b"].copy()
    b[5, 0], b[6, 1], b[7, 2] = CROP_RANGES["box"][0], CROP_RANGES["box"][4], np.nan      # on a face (kept), on a face, NaN (dropped)
    for name, rng in CROP_RANGES.items():
        pts = torch.from_numpy(b)
        ranges = torch.as_tensor(rng, dtype=torch.float32)
        want = torch.prod(torch.logical_and(pts[..., :3] >= ranges[None, :3], pts[..., :3] <= ranges[None, 3:]), dim=-1) > 0
        kept, mask = point_init.crop_to_ranges(_t(b, dev), rng, return_mask=True)
        assert torch.equal(mask.cpu(), want)
        assert torch.equal(kept.cpu(), pts[want])
        print("crop %s: kept %d of %d" % (name, int(want.sum()), len(want)))
        if name == "nothing":
            assert tuple(kept.shape) == (0, 3)
        else:
            assert 0 < int(want.sum()) < len(want) and bool(want[5]) and not bool(want[7])
            assert np.array_equal(point_init.crop_to_ranges(_t(fx["merge_b"], dev), rng).cpu().numpy(), fx["crop_box"])
    assert tuple(point_init.crop_to_ranges(_t(b[:0], dev), CROP_RANGES["box"]).shape) == (0, 3)


def check_group(name, dev):
    """order = the stable argsort of cam_ind, offsets = the cumulative bincount"""
    from pointnerf_amd import point_init
    cam, M = make_group_input(name)
    t = torch.from_numpy(cam)
    order, offsets = point_init.group_by_view(_t(cam, dev), M)
    assert order.dtype == torch.int64 and offsets.dtype == torch.int64 and tuple(order.shape) == (len(cam),) and tuple(offsets.shape) == (M + 1,)
    want_order = torch.argsort(t, stable=True)
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(t, minlength=M), 0)])
    assert torch.equal(offsets.cpu(), want_off)
    assert torch.equal(order.cpu(), want_order)
    again = point_init.group_by_view(_t(cam.astype(np.int32), dev)[:, None], M)
    assert torch.equal(again[0], order) and torch.equal(again[1], offsets)
    if name == "blocks":
        assert int((want_off[1:] == want_off[:-1]).sum()) >= 200          # views without points


def e2e_reference_lists(fx):
    sizes = fx["e2e_sizes"].tolist()
    return fx["e2e_xyz"], fx["e2e_view_ids"], sizes


def check_end_to_end(dev):
    """points_from_cloud (merge at 100, crop, no down-sampling) equals the reference's grouped lists bit for bit"""
    from pointnerf_amd import point_init
    fx = fixture()
    inp = make_e2e_inputs(E2E_CASE)
    for k in ("a", "b", "campos", "camdir"):
        assert np.array_equal(inp[k], fx["e2e_" + k]), k
    xyz, view_ids, offsets, cam_ind = point_init.points_from_cloud([_t(inp["a"], dev), _t(inp["b"], dev)], _t(inp["campos"], dev), _t(inp["camdir"], dev),
                                                                   vox_res=0, ranges=E2E_RANGES, merge_res=E2E_MERGE_RES)
    want_xyz, want_ids, sizes = e2e_reference_lists(fx)
    print("e2e: %d points in %d groups (of %d + %d given)" % (len(want_xyz), len(want_ids), len(inp["a"]), len(inp["b"])))
    assert view_ids.dtype == torch.int64 and offsets.dtype == torch.int64 and cam_ind.dtype == torch.int64
    assert np.array_equal(view_ids.cpu().numpy(), want_ids)
    assert np.array_equal(np.diff(offsets.cpu().numpy()), np.asarray(sizes)) and int(offsets[0]) == 0
    assert np.array_equal(xyz.cpu().numpy(), want_xyz)
    assert np.array_equal(cam_ind.cpu().numpy(), np.repeat(want_ids, sizes))
    assert 0 < len(want_xyz) < len(inp["a"]) + len(inp["b"]) and 1 < len(want_ids) < 24       # merge and crop removed points, some views won none
    # one tensor instead of a list, no merge, no crop: every point, grouped
    xyz1, ids1, off1, cam1 = point_init.points_from_cloud(_t(inp["a"], dev), _t(inp["campos"], dev), _t(inp["camdir"], dev))
    nv = point_init.nearest_view(_t(inp["campos"], dev), _t(inp["camdir"], dev), _t(inp["a"], dev))[:, 0]
    order = torch.argsort(nv.cpu(), stable=True)
    assert torch.equal(xyz1.cpu(), torch.from_numpy(inp["a"])[order]) and torch.equal(cam1.cpu(), nv.cpu()[order])
    assert torch.equal(ids1.cpu(), torch.unique(nv.cpu()))
    # nothing left after the crop
    xyz0, ids0, off0, cam0 = point_init.points_from_cloud(_t(inp["a"], dev), _t(inp["campos"], dev), _t(inp["camdir"], dev), ranges=CROP_RANGES["nothing"])
    assert tuple(xyz0.shape) == (0, 3) and len(ids0) == 0 and off0.tolist() == [0] and len(cam0) == 0


def check_vox_chain(dev):
    """vox_res > 0: the library's own construct_vox_points_closest composed by hand, cloud i at vox_res // 1.5**i"""
    from pointnerf_amd import point_init
    inp, m = make_e2e_inputs(E2E_CASE), make_merge_inputs()
    a, b = _t(m["a"], dev), _t(m["b"], dev)
    cp, cd = _t(inp["campos"], dev), _t(inp["camdir"], dev)
    xyz, ids, off, cam = point_init.points_from_cloud([a, b], cp, cd, vox_res=20, ranges=E2E_RANGES, merge_res=7)
    parts = [point_init.crop_to_ranges(a, E2E_RANGES), point_init.crop_to_ranges(point_init.merge_by_occupancy(a, b, 7), E2E_RANGES)]
    picked = []
    for i, c in enumerate(parts):
        idx = point_init.construct_vox_points_closest(c, 20 // (1.5 ** i))[2]
        assert 0 < len(idx) < len(c)
        picked.append(c[idx])
    allp = torch.cat(picked)
    nv = point_init.nearest_view(cp, cd, allp)[:, 0]
    order = torch.argsort(nv, stable=True)
    assert torch.equal(xyz, allp[order]) and torch.equal(cam, nv[order]) and torch.equal(ids, torch.unique(nv))
    assert torch.equal(off, torch.cat([torch.zeros(1, dtype=torch.int64, device=off.device), torch.cumsum(torch.bincount(nv)[ids], 0)]))


def look_at_c2w(eye, target):
    """camera-to-world [4,4] float64, z forward, y down"""
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, eye
    return M


def embed_setup(dev, default_conf):
    """6 ring cameras, 32 x 40 images with an 8-channel feature map each, the e2e clouds"""
    from pointnerf_amd.mvs_points_model import MvsPointsModel
    V, H, W = 6, 32, 40
    inp = make_e2e_inputs(E2E_CASE)
    pos, _ = cameras("ring", V)
    c2ws = torch.from_numpy(np.stack([look_at_c2w(pos[v].astype(np.float64), np.zeros(3)) for v in range(V)]).astype(np.float32))
    K = torch.tensor([[30.0, 0.0, W / 2], [0.0, 30.0, H / 2], [0.0, 0.0, 1.0]]).expand(V, 3, 3).contiguous()
    g = torch.Generator().manual_seed(5)
    feats = [[torch.rand(1, 3, H, W, generator=g).to(dev), torch.randn(1, 8, H // 2, W // 2, generator=g).to(dev)] for _ in range(V)]
    args = types.SimpleNamespace(depth_occ=0, ref_vid=0, shading_feature_mlp_layer0=0, appr_feature_str0=["imgfeat_0_01", "dir_0", "point_conf"])
    opt = types.SimpleNamespace(vox_res=0, ranges=E2E_RANGES, load_points=3, default_conf=default_conf, resample_pnts=0, point_features_dim=8)
    return MvsPointsModel(args), [_t(inp["a"], dev), _t(inp["b"], dev)], c2ws.to(dev), K.to(dev), (H, W), feats, opt


def check_neural_points(dev):
    """neural_points_from_cloud = points_from_cloud + query_embedding per group by hand, bit for bit; the default_conf scaling"""
    from pointnerf_amd import point_init
    for default_conf in (0.15, -1.0):
        model, clouds, c2ws, K, HDWD, feats, opt = embed_setup(dev, default_conf)
        asked = []
        features_of = lambda v: asked.append(v) or feats[v]
        xyz, emb, color, pdir, conf = point_init.neural_points_from_cloud(model, clouds, c2ws, K, HDWD, features_of, opt)
        campos, camdir = point_init.campos_ray(c2ws, K, HDWD)
        assert torch.allclose(campos, c2ws[:, :3, 3].cpu()) and torch.allclose(camdir.norm(dim=-1), torch.ones(len(camdir)), atol=1e-4)
        assert float((camdir * c2ws[:, :3, 2].cpu()).sum(-1).min()) > 0.99          # the centre ray is (nearly) the optical axis
        gx, ids, off, _ = point_init.points_from_cloud(clouds, campos.to(dev), camdir.to(dev), vox_res=0, ranges=E2E_RANGES, merge_res=100)
        assert asked == ids.tolist() and len(asked) > 1
        N = len(gx)
        assert torch.equal(xyz, gx) and tuple(emb.shape) == (1, N, 8) and tuple(color.shape) == (1, N, 3) and tuple(pdir.shape) == (1, N, 3)
        assert tuple(conf.shape) == (1, N, 1)
        o = off.tolist()
        for g, v in enumerate(ids.tolist()):
            pts, c2w = gx[o[g]:o[g + 1]], c2ws[v]
            w2c = torch.inverse(c2w)
            cam_xyz = (torch.cat([pts, torch.ones_like(pts[..., -1:])], dim=-1) @ w2c.transpose(0, 1))[..., :3]
            e, c, d, cf = model.query_embedding(HDWD, cam_xyz[None], None, feats[v], c2w[None, None], w2c[None, None], K[v][None, None], 0, pointdir_w=True)
            sl = slice(o[g], o[g + 1])
            assert torch.equal(emb[:, sl], e) and torch.equal(color[:, sl], c) and torch.equal(pdir[:, sl], d), v
            assert torch.equal(conf[:, sl], cf * 0.15 if default_conf > 0 else cf), v
        assert float(emb.abs().max()) > 0 and float(color.abs().max()) > 0          # points do project into the images
        assert torch.equal(conf, torch.full_like(conf, 0.15 if default_conf > 0 else 1.0))


def check_reproducible(dev):
    """two runs, the same bits"""
    from pointnerf_amd import point_init
    inp, m = make_nv_inputs("ring24"), make_merge_inputs()
    cp, cd = _t(inp["campos"], dev), _t(inp["camdir"], dev)
    runs = []
    for _ in range(2):
        nv = point_init.nearest_view(cp, cd, _t(inp["xyz"], dev))
        kept, mask = point_init.merge_by_occupancy(_t(m["a"], dev), _t(m["b"], dev), 7, return_mask=True)
        order, offsets = point_init.group_by_view(nv, 24)
        whole = point_init.points_from_cloud([_t(m["a"], dev), _t(m["b"], dev)], cp, cd, ranges=E2E_RANGES, merge_res=7)
        runs.append((nv, kept, mask, order, offsets) + whole)
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert torch.equal(runs[0][0].cpu()[:, 0], torch.from_numpy(run_nearest("ring24", dev)[1]))


def check_refusals(dev):
    """bad M, shapes and types, resample_pnts, the entry points' own errors"""
    import ctypes
    import pytest
    from pointnerf_amd import point_init, _lib as L
    inp = make_nv_inputs("m1")
    xyz, cp, cd = _t(inp["xyz"], dev), _t(inp["campos"], dev), _t(inp["camdir"], dev)
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):                              # M = 0
        point_init.nearest_view(cp[:0], cd[:0], xyz)
    with pytest.raises(ValueError, match="camera"):
        point_init.nearest_view(cp, torch.cat([cd, cd]), xyz)
    for bad in (torch.cat([xyz, xyz[:, :1]], -1), xyz.reshape(-1), xyz[None]):            # [N,4], [3N], [1,N,3]
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            point_init.nearest_view(cp, cd, bad)
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            point_init.points_from_cloud(bad, cp, cd)
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            point_init.merge_by_occupancy(xyz, bad)
    with pytest.raises(ValueError, match="floating-point"):
        point_init.nearest_view(cp, cd, (xyz * 100).int())
    with pytest.raises(ValueError, match="integer"):
        point_init.group_by_view(xyz[:, 0], 3)
    with pytest.raises(ValueError, match="outside"):
        point_init.group_by_view(_t(np.array([0, 1, 5, 2], np.int64), dev), 3)
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
        point_init.group_by_view(_t(np.array([0, 1], np.int64), dev), 0)
    with pytest.raises(RuntimeError, match="too fine"):
        point_init.merge_by_occupancy(xyz, xyz, 2000)
    with pytest.raises(ValueError, match="two clouds"):
        point_init.points_from_cloud(xyz, cp, cd, merge_res=100)
    # other float types are converted, not misread
    assert torch.equal(point_init.nearest_view(cp.double(), cd.double(), xyz.double()), point_init.nearest_view(cp, cd, xyz))
    model, clouds, c2ws, K, HDWD, feats, opt = embed_setup(dev, 0.15)
    opt.resample_pnts = 1
    with pytest.raises(NotImplementedError, match="resample_pnts"):
        point_init.neural_points_from_cloud(model, clouds, c2ws, K, HDWD, lambda v: feats[v], opt)
    # the C ABI itself
    lib = L.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(xyz.data_ptr())                                                 # a valid pointer: nothing is launched on a refusal
    f3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    f6 = (ctypes.c_float * 6)(*([0.0] * 6))
    assert lib.pnerf_nearest_view(one, 10, one, one, 0, one, z) == -1 and lib.pnerf_nearest_view(one, 10, one, one, -3, one, z) == -1
    assert lib.pnerf_nearest_view(one, -1, one, one, 2, one, z) == -1 and lib.pnerf_nearest_view(one, 10, one, one, 2, z, z) == -1
    assert lib.pnerf_nearest_view(z, 0, z, z, 2, z, z) == 0                               # n == 0 touches nothing
    assert lib.pnerf_occupancy_merge_workspace_bytes(10, 2000) == 0 and lib.pnerf_occupancy_merge_workspace_bytes(-1, 10) == 0
    assert lib.pnerf_occupancy_merge_workspace_bytes(10, 0) == 0
    nws = lib.pnerf_occupancy_merge_workspace_bytes(10, 100)
    assert nws >= 100 ** 3 // 8
    mg = lambda kept, ws_bytes, res=100: lib.pnerf_occupancy_merge(one, 10, one, 10, f3, f3, f3, res, kept, one, one, one, ws_bytes, z)
    assert mg(z, nws) == -1 and mg(one, nws - 1) == -2 and mg(one, nws, 0) == -1 and mg(one, nws, 2000) == -4
    assert lib.pnerf_crop_ranges_workspace_bytes(-1) == 0
    cws = lib.pnerf_crop_ranges_workspace_bytes(10)
    assert lib.pnerf_crop_ranges(one, 10, f6, one, one, one, one, cws - 1, z) == -2 and lib.pnerf_crop_ranges(one, 10, None, one, one, one, one, cws, z) == -1
    assert lib.pnerf_group_by_view_workspace_bytes(10, 0) == 0 and lib.pnerf_group_by_view_workspace_bytes(-1, 3) == 0
    assert lib.pnerf_group_by_view_workspace_bytes(2 ** 31, 3) == 0
    gws = lib.pnerf_group_by_view_workspace_bytes(10, 3)
    assert lib.pnerf_group_by_view(one, 10, 3, one, one, one, gws - 1, z) == -2 and lib.pnerf_group_by_view(one, 10, 0, one, one, one, gws, z) == -1
    assert lib.pnerf_group_by_view(one, 10, 3, z, one, one, gws, z) == -1


def check_cpu_tensors_refused():
    """the device path has no CPU implementation"""
    import pytest
    from pointnerf_amd import point_init
    inp = make_nv_inputs("m1")
    xyz, cp, cd = (torch.from_numpy(inp[k]) for k in ("xyz", "campos", "camdir"))
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.nearest_view(cp, cd, xyz)
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.merge_by_occupancy(xyz, xyz)
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.crop_to_ranges(xyz, CROP_RANGES["box"])
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.group_by_view(torch.zeros(4, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.points_from_cloud([xyz, xyz], cp, cd)
    model, clouds, c2ws, K, HDWD, feats, opt = embed_setup("cpu", 0.15)
    with pytest.raises(RuntimeError, match="device tensor"):
        point_init.neural_points_from_cloud(model, clouds, c2ws, K, HDWD, lambda v: feats[v], opt)

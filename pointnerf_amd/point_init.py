"""Point initialisation that feeds the hot path: voxel down-sampling of a raw point cloud into neural-point
positions.  Drop-in for ``models/mvs/mvs_utils.py`` ``construct_vox_points_closest`` (:537-561; called at
run/train_ft_nonstop.py:138-139) and ``construct_vox_points_xyz`` (:503-517; data/scannet_ft_dataset.py:443-444) without
``torch_scatter``: same arguments, same returns (centroids, voxel coordinates in ``torch.unique(dim=0)`` order, index of the
member closest to each centroid), computed by libpnerf_hip.so (csrc/pointinit.hip) deterministically -- the reference's
scatter_mean adds in atomic order, ties of scatter_min are implementation-defined; here sums run in point order and ties go to
the lowest index.  ``partition_xyz`` (voxelise by one cloud, average another) is not used by any reference script and raises.

In front of it, the step from one depth map per view to that raw cloud (run/train_ft.py:96-146; csrc/depthfuse.hip): ``filter_by_masks_gpu``
(models/mvs/filter_utils.py:222-291) and ``alpha_masking`` (models/mvs/mvs_utils.py:573-607) with the reference's signatures and returns,
``depth_consistency`` (the dense per-view maps of the filter) and ``points_from_depth_maps`` (the plain-tensor front door: depth maps in,
points ready for ``MvsPointsModel.query_embedding`` out).  The depth maps are inputs: a depth sensor, this library's own ``ray_geometry``
maps, or ``depth_maps_from_images`` -- the pretrained MVSNet (``depth_estimators.MVSNet``; cost volume, depth regression and the tail of
``gen_points`` in csrc/mvsdepth.hip) on plain tensors, with the relative projection matrices formed as the dataset forms them
(``relative_proj_mats``); ``points_from_images`` is that followed by ``points_from_depth_maps``.

The other route starts from a cloud the user already has (COLMAP, a sensor, or both: ``--load_points 1/2/3``, run/train_ft.py:642-735;
csrc/cloudinit.hip): ``nearest_view`` (:39-48, the reference's signature and return; one thread per point with the camera loop inside
instead of 10 000-point slices of [10000,M,3] temporaries), ``merge_by_occupancy`` (:657-669: the second cloud fills the holes of the first),
``crop_to_ranges`` (:675-680), ``group_by_view`` (:708-710 as one stable permutation), ``points_from_cloud`` (the chain, with the tiered voxel
down-sampling of :683-694 in between) and ``neural_points_from_cloud`` (the chain plus the per-view ``query_embedding`` loop of :718-732:
what ``NeuralPoints.set_points`` takes).  Merge, crop and grouping equal the reference's lines exactly and keep its order; the nearest view
is the float64 argmin wherever the runner-up is farther than the reference's own fp32 rounding reaches.  ``opt.resample_pnts`` raises."""
import ctypes

import torch

from . import _lib as L, ops


def _space(xyz, vox_res, space_min, space_max):
    """The reference's fp32 arithmetic for the cube that is voxelised (mvs_utils.py:541-551)."""
    if space_min is None:
        xyz_min, xyz_max = torch.min(xyz, dim=-2)[0], torch.max(xyz, dim=-2)[0]
        space_edge = torch.max(xyz_max - xyz_min) * 1.05
        xyz_mid = (xyz_max + xyz_min) / 2
        space_min = xyz_mid - space_edge / 2
        vox = (space_edge / vox_res).expand(3)
    else:
        space_min = torch.as_tensor(space_min, dtype=torch.float32, device=xyz.device)
        space_max = torch.as_tensor(space_max, dtype=torch.float32, device=xyz.device)
        vox = (space_max - space_min) / vox_res
    return space_min.float().cpu(), vox.float().cpu()


def _downsample(xyz_val, vox_res, partition_xyz, space_min, space_max):
    if partition_xyz is not None:
        raise NotImplementedError("partition_xyz is outside the hot-path scope (no reference script passes it)")
    if not xyz_val.is_cuda:
        raise RuntimeError("pointnerf_amd: point initialisation runs on the device only (no CPU implementation)")
    xyz = xyz_val.detach().reshape(-1, 3).contiguous().float()
    n, res = xyz.shape[0], int(vox_res)
    smin, vox = _space(xyz, res, space_min, space_max)
    lib = L.lib()
    nws = lib.pnerf_voxel_downsample_workspace_bytes(n, res, res, res)
    if nws == 0:
        raise RuntimeError("pointnerf_amd: vox_res=%d is too fine for 32-bit voxel keys" % res)
    dev = xyz.device
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    cen = torch.empty(n, 3, dtype=torch.float32, device=dev)
    gidx = torch.empty(n, 3, dtype=torch.int32, device=dev)
    midx = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    fa = (ctypes.c_float * 3)
    L.check(lib.pnerf_voxel_downsample(ctypes.c_void_p(xyz.data_ptr()), n, fa(*smin.tolist()), fa(*vox.tolist()), res, res, res,
                                       ctypes.c_void_p(cen.data_ptr()), ctypes.c_void_p(gidx.data_ptr()), ctypes.c_void_p(midx.data_ptr()),
                                       ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nws,
                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "pnerf_voxel_downsample")
    m, outside = (int(v) for v in counts.cpu())
    return cen[:m], gidx[:m], midx[:m], outside


def construct_vox_points_closest(xyz_val, vox_res, partition_xyz=None, space_min=None, space_max=None):
    """-> (xyz_centroid [M,3] f32, sparse_grid_idx [M,3] i32, min_idx [M] i64); mvs_utils.py:537-561."""
    cen, gidx, midx, _ = _downsample(xyz_val, vox_res, partition_xyz, space_min, space_max)
    return cen, gidx, midx


def construct_vox_points_xyz(xyz_val, vox_res, partition_xyz=None, space_min=None, space_max=None):
    """-> xyz_centroid [M,3]; mvs_utils.py:503-517."""
    return _downsample(xyz_val, vox_res, partition_xyz, space_min, space_max)[0]


# ---- depth-map fusion (csrc/depthfuse.hip) ---------------------------------------------------------------------------------------------
def _pair_tables(intrinsics, extrinsics):
    """[V,V,DF_PAIR_FLOATS] fp32 (host): per (reference r, source s) the two reprojections with the intrinsics folded in, formed in float64
    with batched 4 x 4 arithmetic and rounded once (include/pnerf.h, pnerf_depth_consistency)."""
    K = intrinsics.detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    E = extrinsics.detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    V = E.shape[0]
    Kinv, Einv = torch.linalg.inv(K), torch.linalg.inv(E)
    fwd = E[None, :] @ Einv[:, None]                        # [r,s] = E_s E_r^-1
    bwd = E[:, None] @ Einv[None, :]                        # [r,s] = E_r E_s^-1
    T = torch.zeros(V, V, L.DF_PAIR_FLOATS, dtype=torch.float64)
    T[..., 0:9] = (K[None, :] @ fwd[..., :3, :3] @ Kinv[:, None]).reshape(V, V, 9)
    T[..., 9:12] = (K[None, :] @ fwd[..., :3, 3:4]).reshape(V, V, 3)
    RK = bwd[..., :3, :3] @ Kinv[None, :]
    T[..., 12:21] = (K[:, None] @ RK).reshape(V, V, 9)
    T[..., 21:24] = (K[:, None] @ bwd[..., :3, 3:4]).reshape(V, V, 3)
    T[..., 24:27] = RK[..., 2, :]
    T[..., 27] = bwd[..., 2, 3]
    return T.to(torch.float32).contiguous()


def _same_size(shapes):
    if any(tuple(sh) != tuple(shapes[0]) for sh in shapes):
        L.check(-4, "depth fusion (views of different size: %s)" % sorted({tuple(sh) for sh in shapes}))


def depth_consistency(depth, intrinsics, extrinsics):
    """depth [V,H,W], intrinsics [V,3,3], extrinsics [V,4,4] (world to camera) -> (geo_mask_sum [V,H,W] int32: the number of other views
    whose reprojection agrees with the pixel (< 1 pixel, < 1 % depth; filter_utils.py:203-218), depth_avg [V,H,W]: the mean of the pixel's
    depth and the agreeing reprojected depths (:259)).  Useful alone as a per-view confidence map."""
    ops._need_cuda(depth, "depth")
    if depth.dim() != 3:
        raise ValueError("pointnerf_amd: depth must be [V,H,W], got %s" % list(depth.shape))
    dev = depth.device
    d = depth.detach().contiguous().float()
    V, H, W = d.shape
    pairs = _pair_tables(intrinsics, extrinsics)
    if pairs.shape[0] != V:
        raise ValueError("pointnerf_amd: %d depth maps, %d cameras" % (V, pairs.shape[0]))
    pairs = pairs.to(dev)
    geo = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    avg = torch.empty(V, H, W, dtype=torch.float32, device=dev)
    hw = (ctypes.c_int32 * (2 * V))(*([H, W] * V))
    L.check(L.lib().pnerf_depth_consistency(ops._ptr(d), hw, V, ops._ptr(pairs), ops._ptr(geo), ops._ptr(avg), ops._stream()),
            "pnerf_depth_consistency")
    return geo, avg


def _fuse(cam_xyz, confidence, points_mask, intrinsics, extrinsics, depth_conf_thresh, geo_cnsst_num, default_conf, ranges):
    """cam_xyz [V,H,W,3], confidence [V,H,W], points_mask [V,H,W] -> (xyz_cam [n,3], xyz_world [n,3], confidence [n], view_id [n] int32)"""
    dev = cam_xyz.device
    cam = cam_xyz.detach().contiguous().float()
    V, H, W, _ = cam.shape
    geo, avg = depth_consistency(cam[..., 2], intrinsics, extrinsics)
    conf = confidence.detach().to(dev).contiguous().float()
    pmask = (points_mask.detach().to(dev) != 0).to(torch.uint8).contiguous()
    # filter_utils.py:282 inverts the fp32 extrinsics with torch.inverse; here on the host (16 numbers per view)
    inv_ext = torch.inverse(extrinsics.detach().to("cpu", torch.float32).reshape(V, 4, 4)).contiguous().to(dev)
    fa = lambda vals: (ctypes.c_float * len(vals))(*vals)
    factor = None
    if default_conf > 1.0:                                   # reassign_conf (:294-297): torch's own ten values of the factor
        factor = fa((1 - 1.0 / torch.pow(1.14869, torch.arange(1, 11, dtype=torch.int32))).tolist())
    rng = None
    if ranges is not None and ranges[0] > -99.0:             # range_mask_torch (:146-154)
        rng = fa(torch.as_tensor(ranges, dtype=torch.float32).reshape(6).tolist())
    lib = L.lib()
    n = V * H * W
    nws = lib.pnerf_depth_fuse_select_workspace_bytes(V, H, W)
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device=dev)
    xyz_cam = torch.empty(n, 3, dtype=torch.float32, device=dev)
    xyz_world = torch.empty(n, 3, dtype=torch.float32, device=dev)
    conf_out = torch.empty(n, dtype=torch.float32, device=dev)
    view_id = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(lib.pnerf_depth_fuse_select(ops._ptr(geo), ops._ptr(avg), ops._ptr(cam), ops._ptr(conf), ops._ptr(pmask), ops._ptr(inv_ext), V, H, W,
                                        float(depth_conf_thresh), int(geo_cnsst_num), factor, rng, ops._ptr(xyz_cam), ops._ptr(xyz_world),
                                        ops._ptr(conf_out), ops._ptr(view_id), ops._ptr(count), ops._ptr(ws), nws, ops._stream()),
            "pnerf_depth_fuse_select")
    m = int(count.cpu())
    return xyz_cam[:m], xyz_world[:m], conf_out[:m], view_id[:m]


def filter_by_masks_gpu(cam_xyz_all, intrinsics_all, extrinsics_all, confidence_all, points_mask_all, opt, vis=False, return_w=False,
                        cpu2gpu=False, near_fars_all=None):
    """models/mvs/filter_utils.py:222-291: lists over the views of cam_xyz [1,1,C,H,W,3], intrinsics [1,3,3], extrinsics [1,4,4], confidence
    [1,C,H,W], points_mask [1,C,H,W] -> (xyz_cam_lst, xyz_world_lst, confidence_filtered_lst), one entry per view, the kept pixels in
    row-major order.  ``opt``: depth_conf_thresh, geo_cnsst_num, default_conf, ranges, manual_depth_view, far_plane_shift."""
    if opt.manual_depth_view > 1:
        raise NotImplementedError("manual_depth_view > 1 (several depth hypotheses per pixel, no geometric filter) is not on the path of "
                                  "given depth maps")
    if opt.far_plane_shift is not None:
        raise NotImplementedError("far_plane_shift (background points behind the far plane) is not on the path of given depth maps")
    V = len(cam_xyz_all)
    if V < 1:
        L.check(-1, "depth fusion (no views)")
    _same_size([c.shape[-3:-1] for c in cam_xyz_all])
    to = (lambda t: t.cuda()) if cpu2gpu else (lambda t: t)
    H, W = cam_xyz_all[0].shape[-3:-1]
    cam = torch.stack([to(c).reshape(-1, H, W, 3)[0] for c in cam_xyz_all])
    ops._need_cuda(cam, "cam_xyz_all")
    conf = torch.stack([to(c)[0, 0] for c in confidence_all])
    pmask = torch.stack([to(c)[0, 0] for c in points_mask_all])
    K = torch.stack([k[0] for k in intrinsics_all])
    E = torch.stack([e[0] for e in extrinsics_all])
    xyz_cam, xyz_world, cf, vid = _fuse(cam, conf, pmask, K, E, opt.depth_conf_thresh, opt.geo_cnsst_num, opt.default_conf, opt.ranges)
    sizes = torch.bincount(vid.long(), minlength=V).tolist()
    back = (lambda t: t.cpu()) if cpu2gpu else (lambda t: t)
    return tuple([back(p) for p in torch.split(t, sizes)] for t in (xyz_cam, xyz_world, cf))


def alpha_masking(points, alphas, intrinsics, c2ws, w2cs, near_far, opt=None):
    """models/mvs/mvs_utils.py:573-607: points [N,3+] world positions, alphas[i][0] the [H,W] alpha of view i, intrinsics[i] [3,3], w2cs[i]
    [4,4] (c2ws is not read, as there) -> bool [N]: the points every view sees on its foreground (and between near - 1 and far)."""
    ops._need_cuda(points, "points")
    dev = points.device
    host = lambda lst, r, c: torch.stack([torch.as_tensor(a).detach().to("cpu", torch.float32).reshape(r, c) for a in lst]).contiguous()
    V = len(alphas)
    al = [torch.as_tensor(alphas[i][0]) for i in range(V)]
    _same_size([a.shape for a in al])
    H, W = al[0].shape
    alpha = torch.stack([a.to(dev, torch.float32) for a in al]).contiguous()
    K, M = host([intrinsics[i] for i in range(V)], 3, 3).to(dev), host([w2cs[i] for i in range(V)], 4, 4).to(dev)
    pts = points.detach()[..., :3].reshape(-1, 3).contiguous().float()
    n = pts.shape[0]
    use_range = 1 if opt is not None and (opt.alpha_range > 0 or opt.inall_img == 0) else 0
    nf = None
    if near_far is not None:
        nf = (ctypes.c_float * 2)(float(near_far[0] - 1.0), float(near_far[1]))
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    L.check(L.lib().pnerf_alpha_hull(ops._ptr(pts), n, ops._ptr(alpha), ops._ptr(M), ops._ptr(K), V, H, W, use_range, nf, ops._ptr(mask),
                                     ops._stream()), "pnerf_alpha_hull")
    return mask.bool()


def points_from_depth_maps(depth, intrinsics, extrinsics, confidence=None, mask=None, alphas=None, *, geo_cnsst_num, depth_conf_thresh,
                           vox_res=0, ranges=None, near_far=None, default_conf=-1):
    """run/train_ft.py:96-146 on plain tensors: depth [V,H,W], intrinsics [V,3,3], extrinsics [V,4,4] (world to camera), optional confidence
    [V,H,W] (default 1), mask [V,H,W] (default all) and alphas [V,H,W] -> (xyz_world [M,3], confidence [M], view_id [M] int64).  Back-projects
    the maps, keeps the pixels that ``geo_cnsst_num`` other views confirm (``filter_by_masks_gpu``), carves with the alphas
    (``alpha_masking``) and, with ``vox_res > 0``, keeps one point per voxel (``construct_vox_points_closest``)."""
    ops._need_cuda(depth, "depth")
    dev = depth.device
    d = depth.detach().float()
    V, H, W = d.shape
    K = intrinsics.detach().to(dev, torch.float32).reshape(V, 3, 3)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)], dim=-1)                                                  # [H,W,3]
    cam = (torch.einsum("vij,hwj->vhwi", torch.linalg.inv(K.double().cpu()).to(dev), pix) * d.double()[..., None]).float()   # K^-1 [x y 1] d, rounded once
    cam[..., 2] = d                                                                                           # the depth map itself, bit for bit
    conf = torch.ones_like(d) if confidence is None else confidence
    pm = torch.ones_like(d, dtype=torch.bool) if mask is None else mask
    _, xyz_world, cf, vid = _fuse(cam, conf, pm, K, extrinsics, depth_conf_thresh, geo_cnsst_num, default_conf, ranges)
    vid = vid.long()
    if alphas is not None:
        al = torch.as_tensor(alphas).reshape(V, 1, H, W)
        E = extrinsics.detach().to("cpu", torch.float32).reshape(V, 4, 4)
        keep = alpha_masking(xyz_world, al, K.cpu(), None, E, near_far)
        xyz_world, cf, vid = xyz_world[keep], cf[keep], vid[keep]
    if vox_res > 0:
        xyz_world, _, idx = construct_vox_points_closest(xyz_world, vox_res)
        cf, vid = cf[idx], vid[idx]
    return xyz_world, cf, vid


# ---- depth maps from images (csrc/mvsdepth.hip, depth_estimators.MVSNet) ------------------------------------------------------------------
def relative_proj_mats(intrinsics, w2cs, views):
    """The dataset's projection matrices of one init item (data/nerf_synth360_ft_dataset.py:398-400, 506-516) for the views ``views``
    (reference first): P = [K with its first two rows / 4] [R|t] as a 4 x 4, the reference view the identity, every other P_src inv(P_ref);
    formed in float64 on the host -> [len(views),4,4] float32."""
    K = torch.as_tensor(intrinsics).detach().to("cpu", torch.float64).reshape(-1, 3, 3)
    E = torch.as_tensor(w2cs).detach().to("cpu", torch.float64).reshape(-1, 4, 4)
    P = torch.eye(4, dtype=torch.float64).repeat(len(views), 1, 1)
    for j, v in enumerate(views):
        Kq = K[v].clone()
        Kq[:2] = Kq[:2] / 4
        P[j, :3, :4] = Kq @ E[v, :3, :4]
    rel = P @ torch.linalg.inv(P[0])[None]
    rel[0] = torch.eye(4, dtype=torch.float64)
    return rel.to(torch.float32)


def depth_values_of(near_far_depth, n_depth=192):
    """models/mvs/mvs_points_model.py:300-302 in its fp32 arithmetic -> [1,n_depth] on the host"""
    near, far = (torch.tensor(float(v), dtype=torch.float32) for v in near_far_depth)
    return (near + torch.arange(0, n_depth, dtype=torch.float32) * ((far - near) / float(n_depth)))[None, :]


def depth_maps_from_images(mvsnet, images, intrinsics, w2cs, view_id_list, near_far_depth, n_depth=192):
    """images [N,3,H,W] (what the dataset hands the depth estimator: ``mvs_images``), intrinsics [N,3,3] at image resolution, w2cs [N,4,4],
    view_id_list: per depth map the indices of its views, the reference view first (the dataset's ``view_id_list``), near_far_depth = (near,
    far) -> (depth, confidence, mask), each [len(view_id_list),H,W]: ``depth_estimators.MVSNet`` at a quarter of the resolution per reference
    view, then the tail of gen_points (nearest up-sampling, the near / far mask, depths clamped to [near, far]).  The 2-D network runs once
    per image, whatever number of depth maps use it."""
    ops._need_cuda(images, "images")
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError("pointnerf_amd: images must be [N,3,H,W], got %s" % list(images.shape))
    dev = images.device
    H, W = images.shape[-2:]
    dv = depth_values_of(near_far_depth, n_depth).to(dev)
    K = torch.as_tensor(intrinsics).detach().to("cpu", torch.float32).reshape(-1, 3, 3)
    out = []
    with torch.no_grad():
        feats = mvsnet.features_of(images.float())
        for views in view_id_list:
            views = [int(v) for v in views]
            proj = relative_proj_mats(intrinsics, w2cs, views)[None].to(dev)
            d, c = mvsnet.depth_and_confidence(images[views][None], proj, dv, features=feats[views].contiguous())
            xyz, conf, mask = ops.depth_to_cam_points(d[0], c[0], (H, W), near_far_depth, K[views[0]])
            out.append((xyz[0, 0, 0, :, :, 2], conf[0, 0], mask[0, 0]))
    return tuple(torch.stack(t) for t in zip(*out))


def points_from_images(mvsnet, images, intrinsics, w2cs, view_id_list, near_far_depth, n_depth=192, **fusion):
    """``depth_maps_from_images`` followed by ``points_from_depth_maps`` (whose keyword arguments ``fusion`` carries: geo_cnsst_num,
    depth_conf_thresh, alphas, vox_res, ...); view_id_list must hold one entry per image, entry i with image i as its reference view
    -> (xyz_world [M,3], confidence [M], view_id [M] int64)."""
    if len(view_id_list) != images.shape[0] or any(int(v[0]) != i for i, v in enumerate(view_id_list)):
        raise ValueError("pointnerf_amd: points_from_images needs one view list per image, image i first in list i")
    depth, conf, mask = depth_maps_from_images(mvsnet, images, intrinsics, w2cs, view_id_list, near_far_depth, n_depth)
    return points_from_depth_maps(depth, intrinsics, w2cs, conf, mask, **fusion)


# ---- points from an external cloud (csrc/cloudinit.hip) -----------------------------------------------------------------------------
def _cloud(t, name):
    """[N,3] floating point on the device -> contiguous float32; anything else is refused (never reshaped or reinterpreted)"""
    ops._need_cuda(t, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("pointnerf_amd: %s must be [N,3], got %s" % (name, list(t.shape)))
    if not t.is_floating_point():
        raise ValueError("pointnerf_amd: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    return t.detach().float().contiguous()


def _nearest_i32(campos, raydir, xyz):
    pts, cp, cd = _cloud(xyz, "xyz"), _cloud(campos, "campos"), _cloud(raydir, "raydir")
    if cp.shape != cd.shape:
        raise ValueError("pointnerf_amd: %d camera positions, %d camera directions" % (cp.shape[0], cd.shape[0]))
    n, M = pts.shape[0], cp.shape[0]
    cam = torch.empty(n, dtype=torch.int32, device=pts.device)
    L.check(L.lib().pnerf_nearest_view(ops._ptr(pts), n, ops._ptr(cp), ops._ptr(cd), M, ops._ptr(cam), ops._stream()), "pnerf_nearest_view")
    return cam


def nearest_view(campos, raydir, xyz, id_list=None):
    """run/train_ft.py:39-48: campos [M,3] camera centres, raydir [M,3] centre rays, xyz [N,3] -> [N,1] int64: per point the camera with the
    smallest |p - c| / 200 + (1.1 - cos(angle between p - c and the centre ray)), ties to the lowest index (``id_list`` is not read, as there)."""
    return _nearest_i32(campos, raydir, xyz).long().view(-1, 1)


def _kept_rows(src, launch, what):
    """the shared tail of merge and crop: launch(kept, count, mask) -> (kept rows in order, bool mask)"""
    n, dev = src.shape[0], src.device
    kept = torch.empty(n, 3, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    L.check(launch(ops._ptr(kept), ops._ptr(count), ops._ptr(mask)), what)
    return kept[:int(count.cpu())], mask.bool()


def merge_by_occupancy(points_xyz, depth_xyz, filter_res=100, return_mask=False):
    """run/train_ft.py:657-669: the rows of ``depth_xyz`` [Nb,3] that fall into no voxel which holds a point of ``points_xyz`` [Na,3]; the
    ``filter_res``^3 voxels span the first cloud's cube (construct_vox_points_ind, mvs_utils.py:520-534, in its fp32 arithmetic), rows outside
    it are kept.  -> kept rows in their order (and the bool mask [Nb])."""
    a, b = _cloud(points_xyz, "points_xyz"), _cloud(depth_xyz, "depth_xyz")
    res = int(filter_res)
    if res < 1:
        L.check(-1, "occupancy merge (filter_res=%d)" % res)
    lib = L.lib()
    nws = lib.pnerf_occupancy_merge_workspace_bytes(b.shape[0], res)
    if nws == 0:
        raise RuntimeError("pointnerf_amd: filter_res=%d is too fine for a 32-bit occupancy bitmap" % res)
    if a.shape[0]:
        xyz_min, xyz_max = torch.min(a, dim=-2)[0], torch.max(a, dim=-2)[0]                                   # mvs_utils.py:524-531
        space_edge = torch.max(xyz_max - xyz_min) * 1.05
        xyz_mid = (xyz_max + xyz_min) / 2
        space_min, space_max = xyz_mid - space_edge / 2, xyz_mid + space_edge / 2
        vox_a, vox_b = (space_edge / res).expand(3), (space_max - space_min) / res                            # A: the scalar edge; B: :530
    else:                                                                                                     # nothing occupies anything
        space_min, vox_a, vox_b = torch.zeros(3), torch.ones(3), torch.ones(3)
    fa = lambda t: (ctypes.c_float * 3)(*t.float().cpu().tolist())
    ws = torch.empty(nws, dtype=torch.uint8, device=b.device)
    kept, mask = _kept_rows(b, lambda k, c, m: lib.pnerf_occupancy_merge(ops._ptr(a), a.shape[0], ops._ptr(b), b.shape[0], fa(space_min), fa(vox_a),
                                                                         fa(vox_b), res, k, c, m, ops._ptr(ws), nws, ops._stream()),
                            "pnerf_occupancy_merge")
    return (kept, mask) if return_mask else kept


def crop_to_ranges(xyz, ranges, return_mask=False):
    """run/train_ft.py:675-680: the rows with ranges[:3] <= p <= ranges[3:], in order"""
    pts = _cloud(xyz, "xyz")
    rng = (ctypes.c_float * 6)(*torch.as_tensor(ranges, dtype=torch.float32).reshape(6).tolist())
    lib = L.lib()
    nws = lib.pnerf_crop_ranges_workspace_bytes(pts.shape[0])
    if nws == 0:
        L.check(-4, "crop (%d points)" % pts.shape[0])
    ws = torch.empty(nws, dtype=torch.uint8, device=pts.device)
    kept, mask = _kept_rows(pts, lambda k, c, m: lib.pnerf_crop_ranges(ops._ptr(pts), pts.shape[0], rng, k, c, m, ops._ptr(ws), nws, ops._stream()),
                            "pnerf_crop_ranges")
    return (kept, mask) if return_mask else kept


def group_by_view(cam_ind, n_views):
    """cam_ind [N] (or [N,1]) integer in [0, n_views) -> (order [N] int64: points by ascending view, original order inside a view -- a stable
    argsort --, offsets [n_views+1] int64: view v owns order[offsets[v]:offsets[v+1]]); run/train_ft.py:708-710 in one pass."""
    ops._need_cuda(cam_ind, "cam_ind")
    if cam_ind.is_floating_point() or cam_ind.dtype == torch.bool:
        raise ValueError("pointnerf_amd: cam_ind must be an integer tensor, got %s" % cam_ind.dtype)
    cam = cam_ind.detach().reshape(-1).to(torch.int32).contiguous()
    n, M, dev = cam.shape[0], int(n_views), cam.device
    if M < 1:
        L.check(-1, "grouping (n_views=%d)" % M)
    lib = L.lib()
    nws = lib.pnerf_group_by_view_workspace_bytes(n, M)
    if nws == 0:
        L.check(-4, "grouping (%d points, %d views)" % (n, M))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int64, device=dev)
    offsets = torch.empty(M + 1, dtype=torch.int64, device=dev)
    L.check(lib.pnerf_group_by_view(ops._ptr(cam), n, M, ops._ptr(order), ops._ptr(offsets), ops._ptr(ws), nws, ops._stream()),
            "pnerf_group_by_view")
    if int(offsets[M].cpu()) != n:
        raise ValueError("pointnerf_amd: cam_ind holds entries outside [0, %d)" % M)
    return order, offsets


def points_from_cloud(clouds, campos, camdir, *, vox_res=0, ranges=None, merge_res=0):
    """run/train_ft.py:649-710 on plain tensors: ``clouds`` one [N,3] tensor or a list of them (COLMAP points, sensor points, ...), campos /
    camdir [M,3] the cameras' centres and centre rays -> (xyz [N',3] grouped by view, view_ids [G] int64 ascending: the views that won a point,
    offsets [G+1] int64: group g is xyz[offsets[g]:offsets[g+1]], cam_ind [N'] int64 in grouped order).
    ``merge_res > 0`` with two clouds: the second keeps only what falls into no occupied voxel of the first (``load_points == 3``, :657-669);
    ``ranges``: every cloud is cropped (:675-680; skipped when ranges[0] <= -99, as there); ``vox_res > 0``: cloud i keeps the member closest to
    the centroid of each voxel at vox_res // 1.5**i (:683-694, ``points_xyz[sampled_pnt_idx]``); the clouds are concatenated; every point goes
    to its nearest view (:707) and the points are listed view by view in their order (:708-710)."""
    lst = [_cloud(c, "clouds[%d]" % i) for i, c in enumerate(clouds if isinstance(clouds, (list, tuple)) else [clouds])]
    if not lst:
        raise ValueError("pointnerf_amd: no cloud given")
    if merge_res > 0:
        if len(lst) != 2:
            raise ValueError("pointnerf_amd: merge_res needs two clouds (points, depth points), got %d" % len(lst))
        lst[1] = merge_by_occupancy(lst[0], lst[1], merge_res)
    if ranges is not None and ranges[0] > -99.0:
        lst = [crop_to_ranges(c, ranges) for c in lst]
    if vox_res > 0:
        if any(len(c) >= 80000000 for c in lst):
            raise NotImplementedError("clouds of 80 million points and more (the reference strides them, :690) are not supported")
        lst = [c[construct_vox_points_closest(c, vox_res // (1.5 ** i))[2]] if len(c) else c for i, c in enumerate(lst)]
    xyz = torch.cat(lst, dim=0) if len(lst) > 1 else lst[0]
    cam = _nearest_i32(campos, camdir, xyz)
    order, offsets = group_by_view(cam, campos.shape[0])
    won = offsets[1:] > offsets[:-1]
    return xyz[order], torch.nonzero(won).reshape(-1), torch.cat([offsets[:1], offsets[1:][won]]), cam.long()[order]


def campos_ray(c2ws, intrinsics, HDWD):
    """The reference datasets' get_campos_ray (data/nerf_synth360_ft_dataset.py:318-333 over data/data_utils.py:55-69) on the host: c2ws
    [V,4,4], intrinsics [V,3,3] or [3,3], HDWD = (height, width) -> (campos [V,3], camdir [V,3]: the unit ray through the centre pixel)."""
    c2w = torch.as_tensor(c2ws).detach().to("cpu", torch.float32).reshape(-1, 4, 4)
    K = torch.as_tensor(intrinsics).detach().to("cpu", torch.float32).reshape(-1, 3, 3).expand(c2w.shape[0], 3, 3)
    cx, cy = float(int(HDWD[1]) // 2), float(int(HDWD[0]) // 2)
    d = torch.stack([(cx + 0.5 - K[:, 0, 2]) / K[:, 0, 0], (cy + 0.5 - K[:, 1, 2]) / K[:, 1, 1], torch.ones(c2w.shape[0])], dim=-1)
    d = (d[:, None, :] @ c2w[:, :3, :3].transpose(1, 2))[:, 0]
    return c2w[:, :3, 3].contiguous(), (d / (torch.norm(d, dim=-1, keepdim=True) + 1e-5)).contiguous()


def neural_points_from_cloud(mvs_model, clouds, c2ws, intrinsics, HDWD, features_of, opt):
    """run/train_ft.py:649-734 end to end: ``points_from_cloud`` (opt.vox_res, opt.ranges, the merge at 100 when opt.load_points == 3), then
    per view that won points ``mvs_model.query_embedding`` on that view alone (:718-732) with ``features_of(view_id)``: the ``img_feats`` list
    of the single view (level 0 the image [1,3,H,W], levels 1.. its feature maps) on the points' device.  c2ws [V,4,4], intrinsics [V,3,3].
    -> (xyz [N,3], embedding [1,N,C], color [1,N,3], dir [1,N,3], conf [1,N,1]) as ``NeuralPoints.set_points`` takes them; the confidence is
    scaled by opt.default_conf when that lies in (0, 1) (:728)."""
    if getattr(opt, "resample_pnts", 0):
        raise NotImplementedError("resample_pnts (run/train_ft.py:698-704: keep one point or a random subset) is not on this path; no reference "
                                  "script sets it")
    first = clouds[0] if isinstance(clouds, (list, tuple)) else clouds
    ops._need_cuda(first, "clouds")
    dev = first.device
    campos, camdir = campos_ray(c2ws, intrinsics, HDWD)
    xyz, view_ids, offsets, _ = points_from_cloud(clouds, campos.to(dev), camdir.to(dev), vox_res=opt.vox_res, ranges=opt.ranges,
                                                  merge_res=100 if getattr(opt, "load_points", 1) == 3 else 0)
    c2ws = torch.as_tensor(c2ws).detach().to(dev, torch.float32).reshape(-1, 4, 4)
    K = torch.as_tensor(intrinsics).detach().to(dev, torch.float32).reshape(-1, 3, 3).expand(c2ws.shape[0], 3, 3)
    outs, bounds = [], offsets.tolist()
    for g, v in enumerate(view_ids.tolist()):
        pts, c2w = xyz[bounds[g]:bounds[g + 1]], c2ws[v]
        w2c = torch.inverse(c2w)                                                                              # :723
        cam_xyz = (torch.cat([pts, torch.ones_like(pts[..., -1:])], dim=-1) @ w2c.transpose(0, 1))[..., :3]   # :726
        emb, color, pdir, conf = mvs_model.query_embedding(HDWD, cam_xyz[None, ...], None, features_of(v), c2w[None, None, ...],
                                                           w2c[None, None, ...], K[v][None, None, ...], 0, pointdir_w=True)
        conf = conf * opt.default_conf if opt.default_conf > 0 and opt.default_conf < 1.0 else conf          # :728
        outs.append((emb, color, pdir, conf))
    if not outs:
        z = lambda c: torch.zeros(1, 0, c, dtype=torch.float32, device=dev)
        return xyz, z(opt.point_features_dim), z(3), z(3), z(1)
    return (xyz,) + tuple(torch.cat(t, dim=1) for t in zip(*outs))

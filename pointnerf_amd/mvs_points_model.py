"""Initial per-point appearance from GIVEN 2-D maps: the part of ``models/mvs/mvs_points_model.py`` ``MvsPointsModel``
that feeds the hot path and needs no network -- ``extract_2d`` (:198-218) and ``query_embedding`` (:225-259) -- with the reference's
signatures, argument meaning and return arity, computed by libpnerf_hip.so (csrc/embed2d.hip: projection into the source views, in-image /
z-buffer masks of ``homo_warp_nongrid`` / ``homo_warp_nongrid_occ`` models/mvs/mvs_utils.py:299-315,333-369, bilinear ``grid_sample`` of
``extract_from_2d_grid`` :411-421, the per-view unit directions :239-251).  ``img_feats`` -- the source images and the feature pyramid of the
reference's FeatureNet -- are inputs of those two.

A model whose ``args`` carry the reference's ``manual_depth_view`` also builds the networks (``depth_estimators``): ``get_image_features``
(:221-222, the four-level pyramid) and ``gen_points`` (:262-341) for ``manual_depth_view == 1`` -- the pretrained MVSNet, whose cost volume
and depth regression are csrc/mvsdepth.hip -- and ``== 0`` (given ``depths_h``); the tail of ``gen_points`` (nearest up-sampling, near / far
mask, the clamped NDC round trip, back-projection) is one more kernel of that file.  ``load_pretrained_d_est`` (:66-74) keeps its signature.
``manual_depth_view == -1`` or ``> 1``, ``manual_std_depth != 0`` and ``far_plane_shift`` raise, naming the option.  A model built from the
few options ``query_embedding`` needs has no networks: its ``gen_points`` and ``get_image_features`` raise.  Given depth maps become the
candidate points in ``point_init``: ``points_from_depth_maps`` / ``filter_by_masks_gpu`` / ``alpha_masking``.
Batch size 1, like every reference script (``full_src_feat[0, mask[0,:,0], :]``, mvs_utils.py:419)."""
import ctypes
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib as L, ops
from .depth_estimators import MVSNet, PyramidFeatureNet
from .point_init import depth_values_of

feature_str_lst = ['appr_feature_str0', 'appr_feature_str1', 'appr_feature_str2', 'appr_feature_str3']


def _host(t, n):
    a = t.detach().to("cpu", torch.float32).contiguous().reshape(-1)
    assert a.numel() == n, (tuple(t.shape), n)
    return a.tolist()


def premlp_init(opt):
    """models/mvs/mvs_points_model.py:22-35 (the 63 -> point_features_dim MLP some scripts put behind the sampled features; checkpoint keys
    ``premlp.*``).  Default torch initialisation here; the reference applies its ``init_seq`` on top."""
    in_channels, blocks = 63, []
    act = getattr(nn, opt.act_type, None)
    for _ in range(opt.shading_feature_mlp_layer1):
        blocks += [nn.Linear(in_channels, opt.point_features_dim), act(inplace=True)]
        in_channels = opt.point_features_dim
    return nn.Sequential(*blocks)


class MvsPointsModel(nn.Module):
    """``args`` needs: depth_occ, ref_vid, shading_feature_mlp_layer0 (and layer1 / act_type / point_features_dim when > 0),
    appr_feature_str0..3 (lists such as ["imgfeat_0_0123", "dir_0", "point_conf"])."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        # the networks exist only for an ``args`` that carries the reference's ``manual_depth_view`` (:46-53: create_mvs); a model built from
        # the few options query_embedding needs has none, and its gen_points / get_image_features raise
        if hasattr(args, "manual_depth_view"):
            self.FeatureNet = PyramidFeatureNet()
            if args.manual_depth_view >= 1:
                self.MVSNet = MVSNet(refine=False, align_corners=bool(getattr(args, "mvs_align_corners", False)))
                if getattr(args, "pre_d_est", None) is not None:
                    self.load_pretrained_d_est(self.MVSNet, args.pre_d_est)
        if getattr(args, "shading_feature_mlp_layer0", 0) > 0:
            self.premlp = premlp_init(args)

    def load_pretrained_d_est(self, model, pre_d_est):
        """:66-74: the checkpoint's ``model`` dictionary with ``module.`` stripped from every key, loaded strictly"""
        print("loading model {}".format(pre_d_est))
        state_dict = torch.load(pre_d_est, map_location=lambda storage, loc: storage)
        model.load_state_dict(OrderedDict((k[7:], v) for k, v in state_dict["model"].items()))

    # ---- the networks ---------------------------------------------------------------------------------------------------------------
    def get_image_features(self, imgs):
        """:221-222 -> the four-level list of models/mvs/models.py:745-756: [images [V,3,H,W], [V,8,H,W], [V,16,H/2,W/2], [V,32,H/4,W/4]]"""
        if not hasattr(self, "FeatureNet"):
            raise NotImplementedError("this model was built without the 2-D networks (its options carry no manual_depth_view): pass img_feats in")
        ops._need_cuda(imgs, "imgs")
        return self.FeatureNet(imgs[:, :self.args.init_view_num])

    def gen_points(self, batch):
        """:262-341 for ``manual_depth_view == 1`` (the pretrained MVSNet) and ``== 0`` (the batch's ``depths_h``) -> (cam_xyz_lst,
        photometric_confidence_lst, nearfar_mask_lst, HDWD, data_mvs, intrinsics_lst, extrinsics_lst), one list entry per view of
        ``depth_vid``: cam_xyz [1,1,1,H,W,3], confidence [1,1,H,W] (none for given depths, as there), mask [1,1,H,W]."""
        if not hasattr(self, "FeatureNet"):
            raise NotImplementedError("this model was built without the depth estimator (its options carry no manual_depth_view): bring the "
                                      "depth maps and call point_init.points_from_depth_maps (or filter_by_masks_gpu / alpha_masking)")
        args = self.args
        mdv = args.manual_depth_view
        if mdv == -1:
            raise NotImplementedError("manual_depth_view == -1 (the learned probability volume, ProbNet) is not built")
        if mdv > 1:
            raise NotImplementedError("manual_depth_view > 1 (several depth hypotheses per pixel) is not built")
        if getattr(args, "manual_std_depth", 0) != 0:
            raise NotImplementedError("manual_std_depth != 0 (depths drawn around the estimate) is not built: the points would not be reproducible")
        if getattr(args, "far_plane_shift", None) is not None:
            raise NotImplementedError("far_plane_shift (background points behind the far plane) is not built")
        batch.pop("scan", None)
        ops._need_cuda(batch["images"], "batch['images']")
        dev = batch["images"].device
        data_mvs = {k: (v.float().to(dev) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}       # decode_batch (:126-130)
        near_fars, intrinsics = data_mvs["near_fars"], batch["intrinsics"]
        depth_vid = [int(c) for c in args.depth_vid]
        cam_xyz_lst, conf_lst, mask_lst, HDWD = [], [], [], None
        if mdv == 1:
            nfd = ops.host_array(batch["near_fars_depth"])[0]
            # :300-302; the reference fixes 192 planes, ``args.n_depth`` (not one of its options) overrides that
            depth_values = depth_values_of(nfd, int(getattr(args, "n_depth", 192))).to(dev)
            dimgs = data_mvs["mvs_images"] if "mvs_images" in data_mvs else data_mvs["images"]
            views = dimgs[0, :args.init_view_num]
            bproj = data_mvs["proj_mats"][0, torch.as_tensor(depth_vid, dtype=torch.long, device=dev)]          # :308
            with torch.no_grad():
                # :306 expands the same images once per depth view; here FeatureNet runs once per distinct image and the batch items share
                depths, confs = self.MVSNet.depth_and_confidence(views[None].expand(len(depth_vid), -1, -1, -1, -1), bproj,
                                                                 depth_values.expand(len(depth_vid), -1), features=self.MVSNet.features_of(views))
            size = tuple(dimgs.shape[-2:])
        else:
            depths = data_mvs["depths_h"][0][depth_vid]
            confs = torch.ones_like(depths)
            size = tuple(depths.shape[-2:])
        for i, vid in enumerate(depth_vid):
            xyz, conf, mask = ops.depth_to_cam_points(depths[i], confs[i], size, near_fars[0, vid], intrinsics[0, vid])
            cam_xyz_lst.append(xyz)
            mask_lst.append(mask)
            if mdv == 1:
                conf_lst.append(conf)
            HDWD = size
        return (cam_xyz_lst, conf_lst, mask_lst, HDWD, data_mvs, [batch["intrinsics"][:, v, ...] for v in depth_vid],
                [batch["w2cs"][:, v, ...] for v in depth_vid])

    # ---- the path ---------------------------------------------------------------------------------------------------------------------
    def extract_2d(self, img_feats, view_ids, layer_ids, intrinsics, c2ws, w2cs, cam_xyz, HD, WD, cam_vid=0, return_mask=False):
        """-> (out_feats [1,N,sum C of layers != 0 per view], colors [1,N,3 per view] or None); :198-218.  img_feats[lid]: [V,C,H,W]."""
        ops._need_cuda(cam_xyz, "cam_xyz")
        if cam_xyz.shape[0] != 1:
            raise NotImplementedError("extract_2d: batch size 1 (the reference's scatter-back is batch-1 code, mvs_utils.py:419)")
        dev = cam_xyz.device
        xyz = cam_xyz.detach()[0].contiguous().float()
        n, nv = xyz.shape[0], len(view_ids)
        if nv > 8 or nv * len(layer_ids) > 32:
            raise NotImplementedError("extract_2d: at most 8 views / 32 maps per call")
        views = (L.ViewDesc * nv)()
        maps = (L.MapDesc * (nv * len(layer_ids)))()
        keep, fcol, ccol, m = [], 0, 0, 0
        for k, vid in enumerate(view_ids):
            views[k].c2w[:] = _host(c2ws[0, cam_vid], 16)
            views[k].w2c[:] = _host(w2cs[0, vid], 16)
            views[k].intrinsic[:] = _host(intrinsics[0, vid], 9)
            views[k].has_w2c = 0 if vid == cam_vid else 1
            for lid in layer_ids:
                fm = img_feats[lid][vid].detach().contiguous().float()
                if fm.device != dev:
                    raise RuntimeError("pointnerf_amd: img_feats must live on the points' device")
                keep.append(fm)
                C, H, W = fm.shape
                maps[m].d_map, maps[m].view, maps[m].C, maps[m].H, maps[m].W = fm.data_ptr(), k, C, H, W
                maps[m].is_color = 1 if lid == 0 else 0
                maps[m].out_col = ccol if lid == 0 else fcol
                if lid == 0:
                    ccol += C
                else:
                    fcol += C
                m += 1
        occ = 1 if self.args.depth_occ > 0 else 0
        lib = L.lib()
        nws = lib.pnerf_extract_2d_workspace_bytes(n, nv, int(HD), int(WD), occ)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        feats = torch.empty(1, n, fcol, dtype=torch.float32, device=dev)
        colors = torch.empty(1, n, ccol, dtype=torch.float32, device=dev) if ccol else None
        mask = torch.empty(nv, n, dtype=torch.uint8, device=dev) if return_mask else None
        L.check(lib.pnerf_extract_2d(ops._ptr(xyz), n, views, nv, maps, m, int(HD), int(WD), occ, 0.1, ops._ptr(feats), fcol, ops._ptr(colors),
                                     ccol, ops._ptr(mask), ops._ptr(ws), nws, ops._stream()), "pnerf_extract_2d")
        del keep
        if return_mask:
            return feats, colors, mask.bool()
        return feats, colors

    def point_dirs(self, cam_xyz, view_ids, c2ws, w2cs, cam_vid, pointdir_w=False):
        """the "dir" block of query_embedding (:239-251) -> [1,N,3 per view]"""
        ops._need_cuda(cam_xyz, "cam_xyz")
        xyz = cam_xyz.detach()[0].contiguous().float()
        n, nv = xyz.shape[0], len(view_ids)
        ids = torch.as_tensor(list(view_ids), dtype=torch.int64)
        c2w_h, w2c_h = c2ws[0].detach().cpu().float(), w2cs[0].detach().cpu().float()
        pos_cam = (c2w_h[ids, :, 3] @ w2c_h[cam_vid].transpose(0, 1))[..., :3].contiguous()              # :243-245, 4 x 4 host arithmetic
        fa = lambda t, k: (ctypes.c_float * k)(*t.reshape(-1).tolist())
        out = torch.empty(1, n, 3 * nv, dtype=torch.float32, device=xyz.device)
        L.check(L.lib().pnerf_point_dirs(ops._ptr(xyz), n, fa(pos_cam, 3 * nv), nv, fa(c2w_h[cam_vid, :3, :3], 9),
                                         None if pointdir_w else fa(c2w_h[self.args.ref_vid, :3, :3], 9), ops._ptr(out), ops._stream()),
                "pnerf_point_dirs")
        return out

    def query_embedding(self, HDWD, cam_xyz, photometric_confidence, img_feats, c2ws, w2cs, intrinsics, cam_vid, pointdir_w=False):
        """-> (points_embedding, points_colors, points_dirs, points_conf); :225-259"""
        HD, WD = HDWD
        points_embedding, points_dirs, points_conf, points_colors = [], None, None, None
        for feat_str in getattr(self.args, feature_str_lst[cam_vid]):
            if feat_str.startswith("imgfeat"):
                _, view_ids, layer_ids = feat_str.split("_")
                twoD_feats, points_colors = self.extract_2d(img_feats, [int(a) for a in view_ids], [int(a) for a in layer_ids], intrinsics,
                                                            c2ws, w2cs, cam_xyz, HD, WD, cam_vid=cam_vid)
                points_embedding.append(twoD_feats)
            elif feat_str.startswith("dir"):
                points_dirs = self.point_dirs(cam_xyz, [int(a) for a in feat_str.split("_")[1]], c2ws, w2cs, cam_vid, pointdir_w)
            elif feat_str.startswith("point_conf"):
                if photometric_confidence is None:
                    photometric_confidence = torch.ones_like(points_embedding[0][..., 0:1])
                points_conf = photometric_confidence
        points_embedding = torch.cat(points_embedding, dim=-1) if len(points_embedding) > 1 else points_embedding[0]
        if getattr(self.args, "shading_feature_mlp_layer0", 0) > 0:
            points_embedding = self.premlp(torch.cat([points_embedding, points_colors, points_dirs, points_conf], dim=-1))
        return points_embedding, points_colors, points_dirs, points_conf

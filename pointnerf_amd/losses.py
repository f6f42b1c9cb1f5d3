"""The terms of the training loss, each in ONE place: a function of (renderer output dict, gt_image, eps) that returns
(numerator, number of local elements) -- the caller divides by its GLOBAL element count (dist.global_counts) and applies the weight.
The form is picked from the keys the renderer handed out (NeuralPointsRayMarching.forward); dist.hot_path_loss and
MvsPointsVolumetricModel.compute_losses are the two callers.  The fused passes are looked up on ``ops`` at call time."""
import torch

from . import ops


def masked_color(out, gt_image, eps=None):
    """``ray_masked_coarse_raycolor`` (models/base_rendering_model.py:543-551): sum over the hit rays of (colour - gt)^2.  ``out`` is the
    renderer's own dict: dense (``_dense_color`` = (ray colours [R,3], hit flags, number of hit rays): one fused pass, no compaction, no
    boolean-mask index) or compacted (``coarse_raycolor`` [1,R'',3] with ``_hit_index`` / ``ray_mask``)."""
    dc = out.get("_dense_color")
    if dc is not None:
        return ops.color_loss_sum_rays(dc[0], gt_image[0], dc[1]), 3 * dc[2]
    pred = out["coarse_raycolor"][0]
    gt = gt_image[0].index_select(0, out["_hit_index"]) if "_hit_index" in out else gt_image[0][out["ray_mask"][0] > 0]
    return ((pred - gt) ** 2).sum(), pred.numel()


def _geometry_sums(out, gt_depth, gt_mask):
    """both numerators of ops.GeometryLossRays on ``out["_dense_geometry"]`` = (depth_sum, acc, bg_trans, hit flags) of a geometry_grad render,
    formed ONCE per output dict (one pass forward, one backward for the two terms) and kept in it under "_geometry_sums"; a call without
    ``gt_depth`` (the bg term alone) runs with zeros in its place and is not reused by a later call that brings one"""
    dg = out.get("_dense_geometry")
    if not isinstance(dg, tuple):
        raise RuntimeError("pointnerf_amd: the depth / bg loss items need the renderer's differentiable geometry: set net_ray_marching.geometry_grad "
                           "(the model shell does it for depth_loss_items / bg_loss_items)")
    have = out.get("_geometry_sums")
    if have is not None and (gt_depth is None or have[2]):
        return have
    rays = lambda t: t.reshape(-1)
    gd = torch.zeros_like(dg[0]) if gt_depth is None else rays(gt_depth)
    nd, nb = ops.geometry_loss_sums_rays(dg[0], dg[1], dg[2], dg[3], gd, rays(gt_mask))
    out["_geometry_sums"] = (nd, nb, gt_depth is not None)
    return out["_geometry_sums"]


def depth(out, gt_depth, gt_mask):
    """the depth loss item ``coarse_depth`` (models/base_rendering_model.py:610-617: l2loss(coarse_depth * gt_mask, gt_depth * gt_mask) on the
    filled [1,R,1] depth, 0 on a ray that missed): sum over ALL rays of m^2 (d - gt_depth)^2, d = depth_sum / (acc + 1e-6); count = rays"""
    return _geometry_sums(out, gt_depth, gt_mask)[0], int(out["_dense_geometry"][3].numel())


def background(out, gt_mask):
    """the bg loss item ``coarse_is_background`` (models/base_rendering_model.py:619-627: l2loss(coarse_is_background * (1 - gt_mask), 1 - gt_mask)
    on the filled background transmittance, 1 on a ray that missed): sum over ALL rays of (1 - m)^2 (T - 1)^2; count = rays"""
    return _geometry_sums(out, None, gt_mask)[1], int(out["_dense_geometry"][3].numel())


def zero_one(out, gt_image, eps, name="conf_coefficient"):
    """``loss_zero_one`` on ``out[name]`` (models/base_rendering_model.py:630-641): sum of log(v) + log(1 - v), v = clamp(., eps, 1 - eps).
    ``conf_coefficient`` also comes as ``_zero_one_sum`` = (the numerator out of the render node, count) or as ``_zero_one`` = (points_conf,
    dense neighbor table, hit flags, count) for the stand-alone fused pass.  None when the renderer handed out none of them."""
    if name == "conf_coefficient" and "_zero_one_sum" in out:
        return out["_zero_one_sum"]
    if name == "conf_coefficient" and "_zero_one" in out:
        conf, pidx_dense, ray_hit, count = out["_zero_one"]
        return ops.zero_one_conf_sum_rays(conf, pidx_dense, ray_hit, eps), count
    if out.get(name) is None:
        return None
    v = torch.clamp(out[name], eps, 1 - eps)
    return (torch.log(v) + torch.log(1 - v)).sum(), v.numel()

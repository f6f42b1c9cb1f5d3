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

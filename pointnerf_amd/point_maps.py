"""Point attribute maps, picking and image-to-point lifting for render-only passes: what connects a pixel back to the
points that produced it.  No reference counterpart.

Every function renders the view's rays in the chunks of ``eval_loop`` (``pixel_grid`` / ``rays_from_pixels``, as ``render_image`` does),
calls ``model.render_dense(..., train=False)`` per chunk and hands the renderer's dense tensors to ``ops.ray_attributes`` (the operator A and
the pick) or ``ops.lift_to_points`` (its adjoint).  With g[r,s,k] = blend_w[r,s] * weight[r,s,k]:

  render_point_maps   a per-point table seen as an image, the point behind every pixel, and how much of the pixel it carries;
  lift_image          an image (or a painted 2D mask) spread back onto the points, accumulating over views;
  view_contribution   sum of g per point over a set of views: the visibility measure (floaters and never-seen points show as ~0);
  points_from_mass / points_from_pick   boolean [N] selections, exactly what ``editing.compose_parts(inds=...)`` takes.

g carries the normalised distance weight, not the confidence factor of the density; the pick is the largest single (sample, slot) entry of a
ray, not a per-point sum over the ray's samples.  Lifting adds with fp32 atomics and is not bit-reproducible; the maps are.  ``model`` is a
NeuralPointsRayMarching or a model shell that holds one as ``net_ray_marching``; its cut and frame settings apply as in any render-only pass.
Chunk rows are contiguous row-major pixel ranges, so results are written by slice."""
import torch

from . import ops
from .eval_loop import pixel_grid, rays_from_pixels


def _marcher(model):
    return getattr(model, "net_ray_marching", model)


def _n_points(marcher):
    return int(marcher.neural_points.xyz.shape[0])


def _dense_chunks(marcher, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk):
    """(first pixel, blend_w [n,SR], weight [n,SR,K], sample_pidx [n,SR,K], ray_hit [n]) of every chunk of the h x w grid"""
    dev = campos.device
    pix = pixel_grid(h, w, dev)
    for k in range(0, h * w, int(chunk)):
        raydir = rays_from_pixels(pix[:, k:k + chunk], intrinsic.to(dev), camrotc2w)
        t = marcher.render_dense(campos, raydir, camrotc2w, near, far, bg_color, train=False)
        yield k, t[3], t[5], t[7]["sample_pidx"], t[7]["ray_hit"]


@torch.no_grad()
def render_point_maps(model, attr, campos, camrotc2w, intrinsic, h, w, near, far, bg_color=None, chunk=160000):
    """Returns dict(attr [h,w,C] float32 -- ``attr`` [N,C] seen through the render, sum of g attr[point]; omitted for ``attr`` = None --,
    top_point [h,w] int32 -- the point of the ray's largest g, -1 where there is none --, top_contrib [h,w] float32 -- that g --, hit [h,w] bool).
    Pixels whose ray missed are 0 / -1."""
    marcher = _marcher(model)
    n = _n_points(marcher)
    dev = campos.device
    C = 0
    if attr is not None:
        if attr.dim() != 2 or int(attr.shape[0]) != n:
            raise ValueError("pointnerf_amd: attr must be [%d, C] (one row per point), got %s" % (n, list(attr.shape)))
        attr = attr.detach().to(device=dev, dtype=torch.float32).contiguous()
        C = int(attr.shape[1])
    out = dict(top_point=torch.empty(h * w, dtype=torch.int32, device=dev), top_contrib=torch.empty(h * w, dtype=torch.float32, device=dev),
               hit=torch.empty(h * w, dtype=torch.bool, device=dev))
    if attr is not None:
        out["attr"] = torch.empty(h * w, C, dtype=torch.float32, device=dev)
    for k, blend_w, weight, pidx, ray_hit in _dense_chunks(marcher, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk):
        got = ops.ray_attributes(attr, blend_w, weight, pidx, ray_hit, n_points=n)
        m = int(ray_hit.shape[0])
        out["top_point"][k:k + m] = got["top_point"]
        out["top_contrib"][k:k + m] = got["top_contrib"]
        out["hit"][k:k + m] = ray_hit > 0
        if attr is not None:
            out["attr"][k:k + m] = got["attr_sum"]
    return {key: v.view(h, w, C) if key == "attr" else v.view(h, w) for key, v in out.items()}


@torch.no_grad()
def lift_image(model, values, campos, camrotc2w, intrinsic, h, w, near, far, mask=None, out=None, bg_color=None, chunk=160000):
    """Spreads an image onto the points: ``values`` [h,w,C] (C <= 8; None: the mass alone) and the optional ``mask`` [h,w] (float or bool: the
    painted 2D region, the per-ray factor) -> (point_sum [N,C], point_mass [N]) with point_sum[p] += g mask values, point_mass[p] += g mask.
    ``out`` = the pair of an earlier call adds into it, so a loop over views accumulates; None starts from zero."""
    marcher = _marcher(model)
    n = _n_points(marcher)
    dev = campos.device
    flat = None
    if values is not None:
        if values.dim() != 3 or tuple(values.shape[:2]) != (h, w):
            raise ValueError("pointnerf_amd: values must be [%d, %d, C], got %s" % (h, w, list(values.shape)))
        flat = values.detach().to(device=dev, dtype=torch.float32).reshape(h * w, -1).contiguous()
    factor = None
    if mask is not None:
        if tuple(mask.shape) != (h, w):
            raise ValueError("pointnerf_amd: mask must be [%d, %d], got %s" % (h, w, list(mask.shape)))
        factor = mask.detach().to(device=dev, dtype=torch.float32).reshape(h * w).contiguous()
    if out is None:
        out = (torch.zeros(n, 0 if flat is None else int(flat.shape[1]), dtype=torch.float32, device=dev),
               torch.zeros(n, dtype=torch.float32, device=dev))
    for k, blend_w, weight, pidx, ray_hit in _dense_chunks(marcher, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk):
        m = int(ray_hit.shape[0])
        ops.lift_to_points(None if flat is None else flat[k:k + m], None if factor is None else factor[k:k + m], blend_w, weight, pidx, ray_hit,
                           n, out=out)
    return out


@torch.no_grad()
def view_contribution(model, views, h, w, chunk=160000, out=None):
    """point_mass [N] accumulated over an iterable of views (dicts with ``campos``, ``camrotc2w``, ``intrinsic`` [3,3] or [1,3,3], ``near``,
    ``far``): the sum of g over every ray of every view that addresses the point.  Points no view sees -- and floaters in front of nothing --
    stay near 0, which ``points_conf`` alone does not show; pruning by it is left to the caller.  ``out`` = an earlier result adds into it."""
    marcher = _marcher(model)
    mass = out
    for view in views:
        intr = view["intrinsic"]
        intr = intr[0] if intr.dim() == 3 else intr
        pair = None if mass is None else (torch.zeros(_n_points(marcher), 0, dtype=torch.float32, device=mass.device), mass)
        _, mass = lift_image(marcher, None, view["campos"], view["camrotc2w"], intr, h, w, view["near"], view["far"], out=pair,
                             bg_color=view.get("bg_color"), chunk=chunk)
    if mass is None:
        raise ValueError("pointnerf_amd: view_contribution got no views")
    return mass


def points_from_mass(point_mass, threshold):
    """bool [N]: the points whose lifted mass exceeds ``threshold``"""
    return point_mass > threshold


def points_from_pick(top_point_map, mask2d, n_points):
    """bool [N]: the points picked (``render_point_maps``' top_point) by some pixel inside ``mask2d`` [h,w]; one scatter of ones, no atomics"""
    picked = top_point_map.reshape(-1).to(torch.long)
    keep = mask2d.reshape(-1).to(device=picked.device, dtype=torch.bool) & (picked >= 0) & (picked < int(n_points))
    sel = torch.zeros(int(n_points) + 1, dtype=torch.bool, device=picked.device)
    sel[torch.where(keep, picked, torch.full_like(picked, int(n_points)))] = True      # every writer stores the same value; row N is the bin
    return sel[:int(n_points)]

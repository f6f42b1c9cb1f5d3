"""Full-image evaluation on top of the hot path -- what ``test()`` of the reference does around
``model.test()`` (run/train_ft.py:252-414): slice the H x W ray grid into chunks, render each chunk, scatter
``coarse_raycolor`` (after ``fill_invalid``) into a canvas by ``pixel_idx``, score PSNR.

Differences in HOW: the reference renders <= 48^2 = 2304 rays per call (278 calls, 278 voxel-grid rebuilds and a
device->host copy of every chunk for an 800^2 image); here a chunk is as large as the dense query buffers allow
(default 160 000 rays: 4 calls per 800^2 image), the grid is built once, and the canvas and the PSNR stay on the device.
``image_scores`` is the device form of run/evaluate.py's report_metrics (PSNR / SSIM / RMSE of the 8-bit images).
"""
import math

import torch

from .neural_points_volumetric_model import fill_invalid


def pixel_grid(h, w, device):
    """pixel_idx [1, h*w, 2] (px, py), row-major like the datasets' no_crop grid (nerf_synth360_ft_dataset.py:598-613)."""
    py, px = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
    return torch.stack([px.reshape(-1), py.reshape(-1)], dim=-1)[None].float()


def rays_from_pixels(pixel_idx, intrinsic, camrotc2w):
    """get_dtu_raydir with dir_norm=False (data/data_utils.py:55-70) on the device: [1,R,2] -> [1,R,3]."""
    x = (pixel_idx[..., 0] + 0.5 - intrinsic[0, 2]) / intrinsic[0, 0]
    y = (pixel_idx[..., 1] + 0.5 - intrinsic[1, 2]) / intrinsic[1, 1]
    dirs = torch.stack([x, y, torch.ones_like(x)], dim=-1)
    return dirs @ camrotc2w[0].T


def cut_setting(marcher, transmittance_cutoff=None, cutoff_stage=None):
    """Context manager: ``marcher.transmittance_cutoff`` / ``marcher.cutoff_stage`` (NeuralPointsRayMarching: early ray termination of
    render-only passes) set for the duration of a block and restored afterwards; None keeps the current setting."""
    import contextlib

    @contextlib.contextmanager
    def scope():
        prev = (marcher.transmittance_cutoff, marcher.cutoff_stage)
        if transmittance_cutoff is not None:
            marcher.transmittance_cutoff = float(transmittance_cutoff)
        if cutoff_stage is not None:
            marcher.cutoff_stage = int(cutoff_stage)
        try:
            yield marcher
        finally:
            marcher.transmittance_cutoff, marcher.cutoff_stage = prev
    return scope()


def geometry_setting(marcher, on=True):
    """Context manager: ``marcher.ray_geometry`` (NeuralPointsRayMarching: depth and opacity maps of render-only passes) set for the duration of a
    block and restored afterwards."""
    import contextlib

    @contextlib.contextmanager
    def scope():
        prev = marcher.ray_geometry
        marcher.ray_geometry = bool(on)
        try:
            yield marcher
        finally:
            marcher.ray_geometry = prev
    return scope()


GEOMETRY_MAPS = (("depth", "coarse_depth"), ("median_depth", "coarse_median_depth"), ("acc", "coarse_acc"))


class _GeometryCanvases:
    """the three [h, w] maps of one view, filled chunk by chunk through ops.geometry_canvas (one launch per chunk, nothing read in between);
    ``maps()`` reads the library's out-of-range flag -- the one host read -- and hands the canvases out"""

    def __init__(self, h, w, device):
        from . import ops
        self.ops = ops
        words = torch.zeros(3 * h * w + 1, dtype=torch.float32, device=device)          # the canvases and the flag word: one fill
        self.canvas = words[:3 * h * w].view(3, h, w)
        self.flag = words[3 * h * w:].view(torch.int32)

    def fill(self, pixel_idx_i32, ray_mask, full):
        """``full`` = a fill_invalid'ed output with the three keys [1, n, 1]; pixel_idx_i32 [n, 2]; ray_mask [n] int8"""
        d, m, a = (full[key][0, :, 0] for _, key in GEOMETRY_MAPS)
        self.ops.geometry_canvas(pixel_idx_i32, ray_mask, d, m, a, (self.canvas[0], self.canvas[1], self.canvas[2]), flag=self.flag)

    def maps(self):
        self.ops.check_canvas_flag(self.flag)
        return {name: self.canvas[i] for i, (name, _) in enumerate(GEOMETRY_MAPS)}


@torch.no_grad()
def render_image(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk=160000, products=None, transmittance_cutoff=None,
                 cutoff_stage=None, geometry=False):
    """Returns (image [h, w, 3] on the device, ray_mask [h*w] bool).  ``products`` = 2 renders with two MFMA products per multiply-add
    (ops.set_inference_products: ~1.5x less matrix work, ray colour within ~2e-5 of the three-product render; the previous setting is
    restored on return); None keeps the library's current setting.  ``transmittance_cutoff`` = c in (0, 1) renders with early ray
    termination in stages of ``cutoff_stage`` sample slots (``model.transmittance_cutoff`` / ``model.cutoff_stage``, set for this call and
    restored on return: every channel within 1.002 c of the full render; 0 switches it off); None keeps the model's current setting.
    ``geometry`` = True returns (image, ray_mask, maps) with maps = dict(depth, median_depth, acc), [h, w] float32 each: the per-ray depth and
    opacity maps of ``model.ray_geometry`` (set for this call and restored on return), written into the canvases by ops.geometry_canvas, 0 where
    the ray missed.  False (default) launches nothing new and returns the pair."""
    from . import ops
    if transmittance_cutoff is not None or cutoff_stage is not None:
        with cut_setting(model, transmittance_cutoff, cutoff_stage):
            return render_image(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk=chunk, products=products, geometry=geometry)
    if products is not None:
        prev = ops.set_inference_products(products)
        try:
            return render_image(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk=chunk, geometry=geometry)
        finally:
            ops.set_inference_products(prev)
    if geometry:
        with geometry_setting(model, True):
            return _render_chunks(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk, True)
    return _render_chunks(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk, False)


def _render_chunks(model, campos, camrotc2w, intrinsic, h, w, near, far, bg_color, chunk, geometry):
    dev = campos.device
    pix = pixel_grid(h, w, dev)
    canvas = torch.empty(h * w, 3, device=dev)
    hit = torch.empty(h * w, dtype=torch.bool, device=dev)
    if geometry:
        geo, pix_i = _GeometryCanvases(h, w, dev), pix[0].to(torch.int32)
    for k in range(0, h * w, chunk):
        pi = pix[:, k:k + chunk]
        raydir = rays_from_pixels(pi, intrinsic.to(dev), camrotc2w)
        out = model(campos=campos, raydir=raydir, camrotc2w=camrotc2w, pixel_idx=pi, near=near, far=far, bg_color=bg_color,
                    h=h, w=w, intrinsic=intrinsic)
        full = fill_invalid(out, bg_color)
        canvas[k:k + chunk] = full["coarse_raycolor"][0]
        hit[k:k + chunk] = out["ray_mask"][0] > 0
        if geometry:
            geo.fill(pix_i[k:k + chunk], out["ray_mask"][0], full)
    if geometry:
        return canvas.view(h, w, 3), hit, geo.maps()
    return canvas.view(h, w, 3), hit


def depth_points(depth_map, campos, camrotc2w, intrinsic):
    """World positions [n, 3] of the pixels of a [h, w] depth map with depth > 0, in row-major pixel order: campos + depth * raydir with
    ``rays_from_pixels``' un-normalised directions (their camera-z component is 1, so the camera-z depth of render_image's maps IS the ray
    parameter).  Plain tensor plumbing on the map's device; the boolean selection is its one host synchronisation."""
    h, w = int(depth_map.shape[0]), int(depth_map.shape[1])
    dev = depth_map.device
    dirs = rays_from_pixels(pixel_grid(h, w, dev), intrinsic.to(dev), camrotc2w.to(dev))[0]          # [h*w, 3]
    d = depth_map.reshape(-1)
    keep = d > 0
    return campos.to(dev).reshape(1, 3) + d[keep][:, None] * dirs[keep]


def psnr(img, gt):
    """mse2psnr of the reference (utils/visualizer.py:140-155): -10 log10(mse)."""
    mse = torch.mean((img.reshape(-1, 3) - gt.reshape(-1, 3).to(img.device)) ** 2)
    return -10.0 * torch.log10(mse)


SCORE_NAMES = ("psnr", "ssim", "rmse")


@torch.no_grad()
def image_scores(img, gt, metrics=SCORE_NAMES, quantize8=True, data_range=2.0):
    """The scores of ``report_metrics`` (run/evaluate.py:55-61,76) for one [H, W, 3] float32 device image against its ground truth, as a
    dict of 0-d float64 device tensors under the names ``scores.txt`` uses; no host read.  ``quantize8`` scores what the reference
    scores: the images after the 8-bit PNG round trip of utils/visualizer.py:58-59, ``uint8(clip(x, 0, 1) * 255) / 255``.

    psnr = 10 log10(1 / mse) and rmse = sqrt(mse); ssim = ``compare_ssim(gt, img, 11, multichannel=True)``.  The reference passes float
    images and no data_range: skimage's PSNR takes range 1 for non-negative float images while its SSIM (<= 0.18, the versions that accept
    the call) takes the float dtype range, 2.  That inconsistency is kept: ``data_range`` is the SSIM's and defaults to 2, PSNR always uses 1.
    Names outside psnr / ssim / rmse raise NotImplementedError as the reference does; lpips / vgglpips do too, naming the weights they lack."""
    from . import ops
    check_score_names(metrics)
    both = ops.image_metrics(img, gt.to(img.device), win=11, data_range=data_range, quantize8=quantize8)
    mse = both[0]
    value = {"psnr": lambda: 10.0 * torch.log10(1.0 / mse), "ssim": lambda: both[1], "rmse": lambda: torch.sqrt(mse)}
    return {key: value[key]() for key in metrics}


def check_score_names(metrics):
    """NotImplementedError for a name ``image_scores`` does not compute (run/evaluate.py:76; lpips / vgglpips: no weights here)"""
    for key in metrics:
        if key in ("lpips", "vgglpips"):
            raise NotImplementedError("metrics of %s not implemented: LPIPS needs the pretrained %s weights of the lpips package, which this "
                                      "library does not ship" % (key, "AlexNet" if key == "lpips" else "VGG"))
        if key not in SCORE_NAMES:
            raise NotImplementedError("metrics of {} not implemented".format(key))


@torch.no_grad()
def test_views(model, views, opt, height, width, test_num_step=1, chunk=160000, on_view=None, metrics=(), transmittance_cutoff=None,
               cutoff_stage=None, geometry=False):
    """``test()`` of the training / evaluation scripts (run/train_ft.py:252-414, run/test_ft.py:134-274) around the model
    shell: for every ``test_num_step``-th view render all its rays through ``model.set_input / model.test()``, scatter the
    visuals into H x W canvases by ``pixel_idx``, score the items of ``opt.test_color_loss_items``
    (``coarse_raycolor``: MSE of the whole canvas against the ground truth scattered the same way, pixels the view has no
    ray for are 0 in both; ``ray_masked_coarse_raycolor``: MSE over the rays that hit the cloud) and accumulate
    ``mse2psnr`` per view like the Visualizer does (utils/visualizer.py:142-156).

    Returns (psnr of ``opt.test_color_loss_items[0]`` averaged over the views -- the function's return value in the
    reference --, {item: mean loss, item + "_psnr": mean psnr}).  Canvases stay on the device; ``on_view(i, visuals)`` receives
    them (the reference writes PNGs there and afterwards re-reads them for PSNR / SSIM / RMSE -- ``metrics`` below -- and LPIPS,
    which needs pretrained network weights and is outside this path).  The chunk is 160 000 rays instead of <= 48^2.

    ``metrics`` (default none: the result is what it was without the keyword) names scores of ``image_scores``: each view's
    ``coarse_raycolor`` canvas is scored against its ``gt_image`` canvas on the device, and the means over the views are added to the
    returned dict under "psnr" / "ssim" / "rmse", the keys of the reference's ``report_metrics`` (run/evaluate.py:76).  They are read back
    once, after the last view.

    ``transmittance_cutoff`` / ``cutoff_stage``: early ray termination for these renders (``render_image``), set on
    ``model.net_ray_marching`` for the duration of the call and restored afterwards; None keeps the current setting.

    ``geometry`` = True adds ``coarse_depth`` / ``coarse_median_depth`` / ``coarse_acc`` canvases, [height, width] float32, to the visuals handed
    to ``on_view`` (``model.net_ray_marching.ray_geometry``, set for the duration of the call; ops.geometry_canvas fills them); the returned
    scores are what they are without it."""
    check_score_names(metrics)                       # before any view is rendered
    if transmittance_cutoff is not None or cutoff_stage is not None:
        with cut_setting(model.net_ray_marching, transmittance_cutoff, cutoff_stage):
            return test_views(model, views, opt, height, width, test_num_step=test_num_step, chunk=chunk, on_view=on_view, metrics=metrics,
                              geometry=geometry)
    if geometry and not model.net_ray_marching.ray_geometry:
        with geometry_setting(model.net_ray_marching, True):
            return test_views(model, views, opt, height, width, test_num_step=test_num_step, chunk=chunk, on_view=on_view, metrics=metrics,
                              geometry=True)
    model.eval()
    dev = model.device
    items = list(getattr(opt, "test_color_loss_items", ["coarse_raycolor"]))
    acc, count, scores = {}, 0, {}
    for i in range(0, len(views), test_num_step):
        view = views[i]
        raydir = view["raydir"].to(dev)
        pixel_idx = view["pixel_idx"].to(dev)
        pixel_idx = pixel_idx.reshape(pixel_idx.shape[0], -1, pixel_idx.shape[-1])
        total = pixel_idx.shape[1]
        pl = pixel_idx[0].to(torch.long)
        edge = torch.zeros([height, width], dtype=torch.bool, device=dev)
        edge[pl[:, 1], pl[:, 0]] = True
        visuals, ray_masks = {}, []
        if geometry:
            geo, pix_i = _GeometryCanvases(height, width, dev), pl.to(torch.int32)
        for k in range(0, total, chunk):
            data = {kk: vv for kk, vv in view.items() if kk != "gt_mask"}
            data["raydir"] = raydir[:, k:k + chunk, :]
            data["pixel_idx"] = pixel_idx[:, k:k + chunk, :]
            data["gt_image"] = view["gt_image"][:, k:k + chunk, :]
            model.set_input(data)
            model.test()
            pid = pl[k:k + chunk]
            for key, value in model.get_current_visuals(data=data).items():
                if value is None or key == "gt_image":
                    continue
                if key not in visuals:
                    visuals[key] = torch.zeros((height, width, 3), dtype=value.dtype, device=dev)
                visuals[key][pid[:, 1], pid[:, 0], :] = value[0]
            ray_masks.append(model.output["ray_mask"] > 0)
            if geometry:
                geo.fill(pix_i[k:k + chunk], model.output["ray_mask"][0], model.output)
        ray_masks = torch.cat(ray_masks, dim=1)                                   # [1, P]
        if geometry:
            maps = geo.maps()
            visuals.update({key: maps[name] for name, key in GEOMETRY_MAPS})
        gt_rays = view["gt_image"].to(dev).reshape(-1, 3)
        gt_canvas = torch.zeros((height * width, 3), dtype=torch.float32, device=dev)
        gt_canvas[edge.reshape(-1)] = gt_rays            # rays must come in row-major pixel order (the datasets' no_crop grid), :332-333
        visuals["gt_image"] = gt_canvas.reshape(height, width, 3)
        losses = {}
        if "coarse_raycolor" in items:
            losses["coarse_raycolor"] = torch.mean((visuals["coarse_raycolor"].reshape(-1, 3) - gt_canvas) ** 2)
        if "ray_masked_coarse_raycolor" in items:
            pred = visuals["coarse_raycolor"][pl[:, 1], pl[:, 0]][ray_masks[0]]
            losses["ray_masked_coarse_raycolor"] = torch.mean((pred - gt_rays[ray_masks[0]]) ** 2)
        for kk, vv in losses.items():
            acc[kk] = acc.get(kk, 0) + vv
            acc[kk + "_psnr"] = acc.get(kk + "_psnr", 0) + (-10.0 * torch.log(vv) / math.log(10.0))
        if metrics:
            for kk, vv in image_scores(visuals["coarse_raycolor"].float().contiguous(), visuals["gt_image"], metrics=metrics).items():
                scores[kk] = scores[kk] + vv if kk in scores else vv
        count += 1
        if on_view is not None:
            on_view(i, visuals)
    avg = {k: float(v) / max(count, 1) for k, v in acc.items()}
    if scores:
        host = torch.stack([scores[k] for k in scores]).cpu()            # the one host read of the scores, after all views
        avg.update({k: float(host[j]) / max(count, 1) for j, k in enumerate(scores)})
    return avg.get(items[0] + "_psnr"), avg


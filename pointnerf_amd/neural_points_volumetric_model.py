"""Drop-in for ``NeuralPointsRayMarching`` of the reference's ``models/neural_points_volumetric_model.py``
(:220-364) -- THE hot nn.Module (query -> aggregate -> ray_dist -> ray_march -> output dict) -- and for
``fill_invalid`` (:87-123).

``forward(**input)`` takes the reference's kwargs (``campos, raydir, gt_image, bg_color, camrotc2w, pixel_idx, near,
far, focal, h, w, intrinsic, **kargs``) and returns the reference's dict with the reference's shapes
(``coarse_raycolor [1,R'',3]``, ``coarse_point_opacity [1,R'',SR]``, ``coarse_is_background [1,R'',1]``,
``ray_mask [1,R] int8``, ``queried_shading``, ``weight``, ``blend_weight``, ``conf_coefficient``).  Internally
everything runs dense over the R submitted rays inside libpnerf_hip.so; the R'' view is produced by one
boolean row-gather at the very end (the only host sync besides reading the valid-sample count).
``opt.prob==1`` adds the probe outputs of :331-362 (per-ray argmax-opacity sample, its location, nearest-neighbor
distance and weighted average colour/dir/conf/embedding) used by ``probe_hole`` (run/train_ft.py:417-530): they touch
one sample per ray, so they are small gathers on top of the dense render (``pnerf_gather_rows`` for the point rows).
A caller that sets ``fused_probe`` (probe.probe_hole(fused=True)) gets them for all R rays from one ``pnerf_probe_rays`` launch instead
(``_output_forms``).
"""
import os

import torch
import torch.nn as nn

from . import dist as pdist
from . import ops
from .fused import FusedRender


def gradient_clamp(sampled_conf, lo=0.0001, hi=1.0):
    """point_aggregators.py:722-724: clamp forward, identity backward."""
    diff = sampled_conf - torch.clamp(sampled_conf, min=lo, max=hi)
    return sampled_conf - diff.detach()


# PNERF_SPECULATE=0: every training step waits for its counters before it is enqueued (rounds 1-3)
SPECULATE = os.environ.get("PNERF_SPECULATE", "1") != "0"


class _CutStats(dict):
    """``last_stats`` of a cut render: ``n_shaded_samples`` / ``rays_cut`` live in a [4] int32 device tensor that the render wrote behind
    everything else it enqueued; they are read back on first access (of either), so the render itself gets no additional synchronisation."""
    _LAZY = ("n_shaded_samples", "rays_cut")

    def __init__(self, plain, cut_counters):
        super().__init__(plain)
        self._cut_counters = cut_counters
        for k in self._LAZY:
            dict.__setitem__(self, k, None)

    def _resolve(self):
        if self._cut_counters is not None:
            host = self._cut_counters.cpu()
            self._cut_counters = None
            dict.__setitem__(self, "n_shaded_samples", int(host[0]))
            dict.__setitem__(self, "rays_cut", int(host[1]))

    def __getitem__(self, key):
        if key in self._LAZY:
            self._resolve()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        self._resolve()
        return dict.items(self)

    def values(self):
        self._resolve()
        return dict.values(self)

    def __repr__(self):
        self._resolve()
        return dict.__repr__(self)


class NeuralPointsRayMarching(nn.Module):

    def __init__(self, tonemap_func=None, render_func=None, blend_func=None, aggregator=None, is_compute_depth=False,
                 neural_points=None, opt=None, num_pos_freqs=0, num_viewdir_freqs=0, **kwargs):
        super().__init__()
        self.aggregator = aggregator
        self.neural_points = neural_points
        self.opt = opt
        self.num_pos_freqs, self.num_viewdir_freqs = num_pos_freqs, num_viewdir_freqs
        self.render_func, self.blend_func, self.tone_map = render_func, blend_func, tonemap_func
        self.return_depth = is_compute_depth
        self.return_color = True
        if is_compute_depth:
            raise NotImplementedError("compute_depth references an undefined ray_ts in the reference "
                                      "(neural_points_volumetric_model.py:318-322); unsupported (SURVEY.md A.11 iii)")
        if opt is not None:
            if getattr(opt, "which_render_func", "radiance") != "radiance" or getattr(opt, "which_blend_func", "alpha") != "alpha" \
                    or getattr(opt, "which_tonemap_func", "off") != "off":
                raise NotImplementedError("only radiance / alpha / off (every script's setting) is implemented")
        # Early ray termination of render-only passes (ours; the reference shades every valid sample of every hit ray): with a cutoff c in
        # (0, 1) a no-grad render shades each ray front to back in stages of ``cutoff_stage`` sample slots and drops the ray once its
        # transmittance (ray_march's, models/rendering/diff_ray_marching.py:508-554) is below c -- ops.render_forward_cut; every channel of
        # the ray colour stays within 1.002 c of the full render, coarse_is_background of a cut ray is its transmittance at termination.
        # 0 (default): the option is off and every path runs what it ran without it.  ``opt.transmittance_cutoff`` is the initial value.
        self.transmittance_cutoff = float(getattr(opt, "transmittance_cutoff", 0.0) or 0.0) if opt is not None else 0.0
        self.cutoff_stage = 16
        # Depth and opacity maps of render-only passes (ours; the reference's is_compute_depth reads an undefined ray_ts, :318-322, and keeps
        # raising above): when true a no-grad ``forward`` adds coarse_depth (the formula of :321 on ray_march's blend weights, with the
        # camera-z depth of a sample for ray_ts), coarse_median_depth and coarse_acc, [1, R'', 1] each, from ONE ops.ray_geometry launch on
        # the dense tensors the render left on the device.  False (default): nothing is launched and the output dict is what it was.
        # ``opt.ray_geometry`` is the initial value.
        self.ray_geometry = bool(getattr(opt, "ray_geometry", False)) if opt is not None else False
        # Depth and mask supervision (ours): when true the render node hands out the ray's depth_sum = sum_s bw_s z_s, acc =
        # sum_s bw_s and background transmittance as DIFFERENTIABLE outputs (one ops.ray_geometry launch on the tensors the render left on the
        # device; the ray march's backward takes their gradients as further channels, pnerf_render_backward_geom) and ``forward`` passes them
        # to the loss under "_dense_geometry" = (depth_sum, acc, bg_trans, hit flags), dense over the R rays, next to "_dense_color"
        # (losses.depth / losses.background).  Distinct from ``ray_geometry`` (the maps of a render-only pass, still refused under
        # gradients).  False (default): the node has the outputs it had and nothing is launched.  ``opt.geometry_grad`` is the initial value.
        self.geometry_grad = bool(getattr(opt, "geometry_grad", False)) if opt is not None else False
        self.last_stats = None
        self._last_camera = None
        self._last_geometry = None
        self._pool_rays = 0
        self._pinned_words = None

    def _host_words(self, n):
        """pinned host memory for the step's asynchronous read-back of its counters"""
        if self._pinned_words is None or self._pinned_words.numel() != n:
            self._pinned_words = torch.empty(n, dtype=torch.int64).pin_memory()
        return self._pinned_words

    def _cut_setting(self, train):
        """(cutoff, stage) when this render takes the cut route (a render-only pass with transmittance_cutoff > 0), None when the option is
        off; refuses the passes that need every sample shaded"""
        if not self.transmittance_cutoff:
            return None
        cut = ops.check_cutoff(self.transmittance_cutoff, self.cutoff_stage)
        if train:
            raise NotImplementedError("transmittance_cutoff = %g is render-only: a training forward (gradients enabled, or train=True) shades every "
                                      "sample -- run the render under torch.no_grad() or set transmittance_cutoff back to 0" % cut[0])
        if getattr(self.opt, "prob", 0) == 1 or bool(getattr(self, "fused_probe", False)):
            raise NotImplementedError("transmittance_cutoff = %g with the probe outputs (opt.prob == 1 / fused_probe): they need the maximum opacity over "
                                      "ALL samples of a ray -- set transmittance_cutoff back to 0 for the probe pass" % cut[0])
        return cut

    def _geometry_setting(self, train):
        """whether this render's ``forward`` adds the depth and opacity maps (``ray_geometry``); refuses the passes they are not defined for"""
        if not self.ray_geometry:
            return False
        if train:
            raise NotImplementedError("ray_geometry is render-only: the depth and opacity maps have no backward, and a training forward (gradients "
                                      "enabled, or train=True) would hand out keys a loss could pick up -- run the render under torch.no_grad() or "
                                      "set ray_geometry back to False")
        if getattr(self.opt, "prob", 0) == 1 or bool(getattr(self, "fused_probe", False)):
            raise NotImplementedError("ray_geometry with the probe outputs (opt.prob == 1 / fused_probe): the probe pass has its own output form "
                                      "-- set ray_geometry back to False for the probe pass")
        return True

    def _geometry_grad_setting(self):
        """whether this render hands out the differentiable geometry (``geometry_grad``); refuses the render-only options it has no meaning with"""
        if not self.geometry_grad:
            return False
        if self.transmittance_cutoff:
            raise NotImplementedError("geometry_grad with transmittance_cutoff = %g: the cut render is render-only and leaves the samples behind the "
                                      "cut unshaded -- set transmittance_cutoff back to 0" % float(self.transmittance_cutoff))
        npnt = self.neural_points
        if isinstance(npnt.Rw2c, torch.Tensor) and npnt.Rw2c.dim() == 3:
            raise NotImplementedError("geometry_grad with one Rw2c frame per point (a composed scene): per-point frames are render-only -- set "
                                      "geometry_grad back to False")
        if getattr(self.opt, "prob", 0) == 1 or bool(getattr(self, "fused_probe", False)):
            raise NotImplementedError("geometry_grad with the probe outputs (opt.prob == 1 / fused_probe): the probe pass has its own output form "
                                      "-- set geometry_grad back to False for the probe pass")
        return True

    def render_dense(self, campos, raydir, camrotc2w, near, far, bg_color=None, train=None, zero_one_eps=None):
        """The fused step on all R rays.  Returns (ray_color [R,3], opacity, bg_trans, blend_w, decoded, weight, zo_sum, dense); zo_sum =
        the zero-one regulariser's numerator over the hit rays' conf_coefficient when a training step is given ``zero_one_eps`` (the
        "render" form of ``_output_forms``; else a constant 0).
        With ``transmittance_cutoff`` > 0 a render-only pass (``train`` false) takes the cut route (``_cut_setting``): samples that were not
        shaded are 0 in opacity / blend_w / decoded / weight, bg_trans of a cut ray is its transmittance at termination (not the full
        render's value), and ``last_stats`` carries ``n_shaded_samples`` / ``rays_cut``."""
        opt, npnt, agg = self.opt, self.neural_points, self.aggregator
        train = torch.is_grad_enabled() if train is None else train
        geometry_grad = self._geometry_grad_setting()
        cut = self._cut_setting(train)
        self._geometry_setting(train)
        # xyz_grad > 0: the point positions are a leaf of the fused step (d xyz from k_agg_backward's XYZG instances)
        xyz_leaf = bool(train) and npnt.xyz.requires_grad
        # one Rw2c frame PER POINT (a composed scene, pointnerf_amd.editing): the table goes to the kernels as a device pointer
        # (pnerf_points.frames) -- it is never read back to the host -- and is render-only, like the reference's frozen Rw2c
        frames = None
        if isinstance(npnt.Rw2c, torch.Tensor) and npnt.Rw2c.dim() == 3:
            ops.frames_are_render_only(npnt.Rw2c, train, " (xyz_grad > 0 included)" if xyz_leaf else "")
            frames = ops.frames_table(npnt.Rw2c, npnt.xyz.shape[0])
        R = raydir.reshape(-1, 3).shape[0]
        if train and self._pool_rays < R:              # worst case (every ray hits): ~16 live [R,SR,K] fp32 tensors around the loss
            ops.reserve_pool(16 * R * int(opt.SR) * int(opt.K) * 4, raydir.device)
            self._pool_rays = R
        dense = npnt.query_dense(dict(campos=campos, raydir=raydir, near=near, far=far))
        # data-parallel callers that exchange touched rows only (dist.plan_sparse_exchange) prepare the row list here, so that its two
        # counts travel with the one host read below instead of synchronising a second time after the backward
        plan = getattr(self, "plan_sparse", None)
        if plan is not None and xyz_leaf:
            raise NotImplementedError("xyz_grad > 0 with the sparse-row gradient exchange (dist.plan_sparse_exchange): the point positions' "
                                      "gradient is not part of the touched-row exchange; use the dense all-reduce (dist.allreduce_grads)")
        plan = plan(dense) if (plan is not None and train) else None
        words = dense["counters"].to(torch.int64) if plan is None else torch.cat([dense["counters"].to(torch.int64), plan[1]])
        st = agg.mlp_state()
        rw = ops.host_array(npnt.Rw2c) if (isinstance(npnt.Rw2c, torch.Tensor) and frames is None) else None
        cam = ops.make_camera(ops.host_array(campos).reshape(-1)[:3], ops.host_array(camrotc2w).reshape(-1)[:9],
                              opt.vsize[2], opt.raydist_mode_unit,
                              bg=None if bg_color is None else ops.host_array(bg_color).reshape(-1)[:3], rw2c=rw)
        self._last_camera = cam
        mlp_params, layout = agg.ordered_params()
        env = dict(cam=cam, xyz=npnt.xyz.detach().reshape(-1, 3).contiguous(), raydir=raydir.detach().reshape(-1, 3).contiguous().float(),
                   dense=dense, R=R, SR=int(opt.SR), K=int(opt.K), n_valid=0, flat=st.flat, packed=st.packed_image(),
                   train=bool(train), layout=layout, want_grad_event=bool(train) and raydir.is_cuda and pdist.active())
        if train and zero_one_eps is not None:
            env["zero_one_eps"] = float(zero_one_eps)
        if xyz_leaf:
            env["xyz_grad"] = True
        if frames is not None:
            env["frames"] = frames
        if cut is not None:
            env["cut"] = cut
        if geometry_grad:
            env["geometry_grad"] = True
        leaves =(npnt.points_embeding, npnt.points_conf, npnt.points_dir, npnt.points_color) + ((npnt.xyz,) if xyz_leaf else ()) + tuple(mlp_params)
        # The step's one host read (number of valid samples: sizes the activation arena; number of hit rays: shapes of the outputs).
        # Round 4: a TRAINING step whose arena already exists is enqueued BEFORE that read with the arena's capacity as the bound -- every
        # kernel takes the actual counts from the device (`counters`, the class partition's tile counts), the host number is only "how much
        # scratch is there" -- so the device starts the aggregator right behind the query instead of idling through the host's wake-up and
        # its ~20 launches (0.2-0.3 ms per step in the kernel trace).  The counts arrive in pinned memory meanwhile; should they exceed the
        # capacity (a batch larger than every one before it), the speculative result is dropped and the step runs again after the arena grew.
        cap = ops.ARENA.capacity_samples(env["K"], raydir.device) if (train and raydir.is_cuda and SPECULATE) else 0
        out = None
        if cap > 0:
            host = self._host_words(words.numel())
            host.copy_(words, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()
            env["n_valid"] = cap
            out = FusedRender.apply(env, *leaves)
            ready.synchronize()
            got = host.clone()
        else:
            got = words.cpu()                                 # the one sync
        n_valid = int(got[0])
        dropped = out is not None and n_valid > cap
        if dropped:                                           # (rare: the arena has to grow; nothing of the dropped result is used)
            ops.ARENA.give(env.pop("_saved", None))
            out, env = None, dict(env)
        if plan is not None:
            self.sparse_plan = (plan[0], int(got[8]), int(got[9]))
        self.last_stats = dict(n_valid_samples=n_valid, rays_hit=int(got[1]), n_selected=int(got[2]), n_neighbor_rows=int(got[3]), rays=R,
                               enqueued_before_host_read=out is not None, speculative_result_dropped=dropped,
                               n_shaded_samples=n_valid, rays_cut=0)
        if out is None:
            env["n_valid"] = n_valid
            out = FusedRender.apply(env, *leaves)
        if cut is not None:                                   # the two counts of the cut render: on the device until somebody asks
            self.last_stats = _CutStats(self.last_stats, env["cut_counters"])
        # geometry_grad: the node's eighth and ninth output (depth_sum, acc) stay behind for ``forward``; the tuple keeps its eight places
        self._last_geometry = tuple(out[7:9]) if geometry_grad else None
        return tuple(out[:7]) + (dense,)

    def _output_forms(self):
        """THE decision of one ``forward`` call, from the caller's flags and the options: (dense colours handed out?, form of the zero-one
        regulariser on conf_coefficient, probe outputs from the fused pass?).

        ``fused_zero_one`` / ``fused_color_loss`` (ours; set by callers whose loss goes through dist.hot_path_loss, and by the model shell of this
        package -- fused_color_loss when every colour-loss item with a non-zero weight is a ray_masked / ray_miss one, the lego script's setting:
        MvsPointsVolumetricModel.create_network_models) say that the only consumer of conf_coefficient / of the rendered colours is the loss.
        Zero-one forms: "render" -- a training step: the numerator is an output of the render node, its conf gradient rides on the node's own conf
        atomics ("_zero_one_sum"); "pass" -- the same caller under no_grad: what the stand-alone fused pass needs, (points_conf, the DENSE neighbor
        table, the rays' hit flags, number of conf_coefficient elements), no [R'', SR, K] copy of the table ("_zero_one", ops.zero_one_conf_sum_rays);
        "tensor" -- weight / blend_weight / conf_coefficient [1, R'', SR, K] materialised like the reference (some other consumer: the sparse
        loss, the probe outputs, a caller without the flag); None -- nobody reads them.
        Dense colours: a TRAINING step gets the dense ray colours and the hit flags under "_dense_color" (ops.ColorLossRays: one pass forward, one
        backward, d colour written for every ray) and the compacted [1, R'', ...] outputs are not formed -- no argsort, no index_selects, no
        scatter-back in the backward (~25 launches per step).
        ``fused_probe`` (ours; set by probe.probe_hole(fused=True) for the duration of its call) says that the only consumer of an ``opt.prob == 1``
        forward is the probe pass: under no_grad the third element is True and the forward hands out the dense colour form plus "_dense_probe", the
        seven probe outputs for all R rays from ONE ops.probe_rays launch -- no argsort / index_select route, no weight / blend_weight /
        conf_coefficient [1, R'', SR, K] copies, no boolean-mask index; fill_invalid(prob=1) only adds the batch axis."""
        opt, grad = self.opt, torch.is_grad_enabled()
        if bool(getattr(self, "fused_probe", False)) and getattr(opt, "prob", 0) == 1 and not grad:
            return True, None, True
        loss_only = bool(getattr(self, "fused_zero_one", False)) and opt.sparse_loss_weight <= 0 and getattr(opt, "prob", 0) == 0
        has_item = "conf_coefficient" in getattr(opt, "zero_one_loss_items", ())
        if has_item and loss_only:
            zero_one = "render" if grad else "pass"
        else:
            zero_one = "tensor" if (has_item or opt.sparse_loss_weight > 0 or getattr(opt, "prob", 0) != 0) else None
        return bool(getattr(self, "fused_color_loss", False)) and grad and loss_only, zero_one, False

    def forward(self, campos, raydir, gt_image=None, bg_color=None, camrotc2w=None, pixel_idx=None, near=None, far=None,
                focal=None, h=None, w=None, intrinsic=None, **kargs):
        opt = self.opt
        if "bg_ray" in kargs:
            bg_color = None
        dense_color, zero_one, fused_probe = self._output_forms()
        ray_color, opacity, bg_trans, blend_w, decoded, weight, zo_sum, dense = self.render_dense(
            campos, raydir, camrotc2w, near, far, bg_color, zero_one_eps=getattr(opt, "zero_epsilon", 1e-3) if zero_one == "render" else None)
        hit = dense["ray_hit"] > 0
        SR, K = int(opt.SR), int(opt.K)
        # Indices of the hit rays WITHOUT a host round trip: their number is already on the host (the counters the arena was
        # sized from), so a stable sort of the 0/1 flags yields them in ascending order.  Boolean-mask indexing would
        # synchronise once per tensor (nonzero), and the device would idle between forward, loss and backward while the
        # host catches up; with this the whole step is enqueued behind one synchronisation.
        n_hit = self.last_stats["rays_hit"]
        if dense_color:
            output = {"_dense_color": (ray_color, dense["ray_hit"], n_hit), "ray_mask": hit.to(torch.int8)[None],
                      "_dense_aux": (opacity.detach(), bg_trans.detach())}       # (for fill_invalid's full-size visuals: references, no work)
        else:
            idx = torch.argsort(dense["ray_hit"], descending=True, stable=True)[:n_hit]
            take = lambda t: t.index_select(0, idx)
            output = {"_hit_index": idx}
            # queried_shading = not any(ray_valid) per ray (:322 of the reference): the R'' rays ARE the rays with a valid sample (ray_mask comes from
            # the same neighbor table, query_worldcoords.cu:425-429), so it is identically zero -- no pass over the [R'', SR] counts
            output["queried_shading"] = torch.zeros(1, n_hit, 3, dtype=torch.float32, device=ray_color.device)
            output["coarse_raycolor"] = take(ray_color)[None]
            output["coarse_point_opacity"] = take(opacity)[None]
            output["coarse_is_background"] = take(bg_trans)[None, :, None]
            output["ray_mask"] = hit.to(torch.int8)[None]
        if zero_one == "render":
            output["_zero_one_sum"] = (zo_sum, n_hit * SR * K)
        elif zero_one == "pass":
            output["_zero_one"] = (self.neural_points.points_conf, dense["sample_pidx"], dense["ray_hit"], n_hit * SR * K)
        elif zero_one == "tensor":                # (never together with the dense colours: those imply a caller that reads conf_coefficient for the loss only)
            output["weight"] = take(weight)[None].detach()
            output["blend_weight"] = take(blend_w)[None, ..., None].detach()
            conf = self.neural_points.points_conf
            pidx_hit = take(dense["sample_pidx"])
            output["conf_coefficient"] = gradient_clamp(ops.gather_rows(conf.reshape(-1, 1), pidx_hit)[..., 0])[None]
        if fused_probe:
            if n_hit > 0:                         # (a batch that hit nothing carries no probe outputs, like the compacted form below)
                npnt = self.neural_points
                rows = lambda t: t.detach().reshape(-1, t.shape[-1]).contiguous()
                pts = ops.make_points(rows(npnt.xyz), rows(npnt.points_embeding), rows(npnt.points_conf), rows(npnt.points_dir), rows(npnt.points_color))
                output["_dense_probe"] = ops.probe_rays(pts, opacity.detach(), weight.detach(), dense["sample_loc"], dense["sample_pidx"], dense["ray_hit"],
                                                        hit.shape[0], SR, K)
        elif getattr(opt, "prob", 0) == 1 and output["coarse_point_opacity"].shape[1] > 0:
            self._probe_outputs(output, dense, hit)
        geometry, self._last_geometry = self._last_geometry, None     # (not kept on the module: the tensors hold the step's graph)
        if geometry is not None:
            # geometry_grad: dense over the R rays and differentiable, for losses.depth / losses.background (a render-only ``ray_geometry``
            # pass below replaces it with its own maps)
            output["_dense_geometry"] = (geometry[0], geometry[1], bg_trans, dense["ray_hit"])
        if self._geometry_setting(torch.is_grad_enabled()):
            # (the camera record render_dense has just built: the kernel reads its position and rotation only)
            geo = ops.ray_geometry(self._last_camera, dense["sample_loc"], dense["sample_nn"], dense["ray_hit"], opacity.detach(), blend_w.detach())
            rows = geo["_rows"].index_select(1, output["_hit_index"])              # ONE gather for the three maps, like the other compacted outputs
            for key, name in GEOMETRY_KEYS:
                output[key] = rows[ops.RAY_GEOMETRY_KEYS.index(name)][None, :, None]
            # the kernel's own full-size results (zeros for the misses already): fill_invalid hands these out instead of scattering the
            # compacted keys back -- references, no work (like "_dense_probe")
            output["_dense_geometry"] = geo
        return output

    def _probe_outputs(self, output, dense, hit):
        """neural_points_volumetric_model.py:331-362, same keys and shapes."""
        npnt = self.neural_points
        with torch.no_grad():
            op = output["coarse_point_opacity"][0]                                   # [R'',SR]
            mx, ind = torch.max(op, dim=-1, keepdim=True)                            # [R'',1]
            output["ray_max_shading_opacity"] = mx[None]
            loc_w = dense["sample_loc"][hit]                                         # [R'',SR,3]
            sel = lambda t: torch.gather(t, 1, ind.view(-1, 1, *([1] * (t.dim() - 2))).expand(-1, 1, *t.shape[2:])).squeeze(1)
            loc_max = sel(loc_w)                                                     # [R'',3]
            output["ray_max_sample_loc_w"] = loc_max[None]
            w = sel(output["weight"][0] * output["conf_coefficient"][0].detach())    # [R'',K]
            pidx = sel(dense["sample_pidx"][hit])                                    # [R'',K]  (-1 slots read point 0, as :708)
            g = lambda t: ops.gather_rows(t.detach().reshape(-1, t.shape[-1]), pidx)  # [R'',K,C]
            xyz_max = g(npnt.xyz)
            output["ray_max_far_dist"] = torch.min(torch.norm(xyz_max - loc_max[:, None, :], dim=-1), dim=-1, keepdim=True)[0][None]
            wk = w[..., None]
            output["shading_avg_color"] = torch.sum(g(npnt.points_color) * wk, dim=-2)[None]
            output["shading_avg_dir"] = torch.sum(g(npnt.points_dir) * wk, dim=-2)[None]
            output["shading_avg_conf"] = torch.sum(g(npnt.points_conf) * wk, dim=-2)[None]
            output["shading_avg_embedding"] = torch.sum(g(npnt.points_embeding) * wk, dim=-2)[None]


# output key of forward / fill_invalid -> name in ops.ray_geometry's dict
GEOMETRY_KEYS = (("coarse_depth", "depth"), ("coarse_median_depth", "median_depth"), ("coarse_acc", "acc"))
PROBE_KEYS = ("ray_max_sample_loc_w", "ray_max_shading_opacity", "shading_avg_color", "shading_avg_dir", "shading_avg_conf",
              "shading_avg_embedding", "ray_max_far_dist")


def fill_invalid(output, bg_color, tonemap_func=None, bg_ray=None, prob=0):
    """neural_points_volumetric_model.py:87-123: scatter the hit rays' results back to all R submitted rays (missed rays get
    the background colour / transmittance 1 / opacity 0; with ``prob == 1`` the probe outputs are zero-filled, :121-122
    ``unmask``).  ``bg_ray`` [B,R,3] replaces the constant background like :104-106."""
    ray_mask = output["ray_mask"]
    B, OR = ray_mask.shape
    if "_dense_color" in output:
        # the fused-colour-loss form of a training step (NeuralPointsRayMarching.forward): the renderer's results are DENSE over the R rays
        # already, so "filling" is a select per ray -- no scatter, no index tensor.  The filled tensors are detached: the colour loss takes
        # its gradient through ops.ColorLossRays on the dense colours (MvsPointsVolumetricModel.compute_losses), these are the visuals.
        ray_color, ray_hit, _ = output["_dense_color"]
        opacity, bg_trans = output["_dense_aux"]
        dev = ray_color.device
        hitb = (ray_hit > 0)
        bgt = torch.where(hitb, bg_trans, torch.ones((), dtype=torch.float32, device=dev))[None, :, None]
        if bg_ray is not None:
            col = bgt * bg_ray.to(dev) + torch.where(hitb[:, None], ray_color.detach(), torch.zeros((), dtype=torch.float32, device=dev))[None]
        else:
            bg = torch.ones([OR, 3], dtype=torch.float32, device=dev) * bg_color.to(dev).reshape(-1, 3)
            if tonemap_func is not None:
                bg = tonemap_func(bg)
            col = torch.where(hitb[:, None], ray_color.detach(), bg)[None]
        op = torch.where(hitb[:, None], opacity, torch.zeros((), dtype=torch.float32, device=dev))[None]
        qs = torch.where(hitb[:, None], torch.zeros((), dtype=torch.float32, device=dev), torch.ones([OR, 3], dtype=torch.float32, device=dev))[None]
        out = dict(output)
        out.update(coarse_is_background=bgt, coarse_mask=1 - bgt, coarse_raycolor=col, coarse_point_opacity=op, queried_shading=qs)
        if prob == 1 and "_dense_probe" in output:
            # the fused probe form: ops.probe_rays has written every ray's row already, zeros for the misses (:121-122 "unmask")
            for k in PROBE_KEYS:
                out[k] = output["_dense_probe"][k][None]
        return out
    sel = output["_hit_index"] if "_hit_index" in output else ray_mask[0] > 0      # index tensor: no nonzero() synchronisation
    dev = output["coarse_raycolor"].device
    bgt = torch.ones([B, OR, 1], dtype=torch.float32, device=dev)
    bgt[0, sel] = output["coarse_is_background"][0]
    if bg_ray is not None:
        col = bgt * bg_ray.to(dev)
        col[0, sel] = col[0, sel] + output["coarse_raycolor"][0]
    else:
        col = torch.ones([B, OR, 3], dtype=torch.float32, device=dev) * bg_color[None, ...].to(dev)
        if tonemap_func is not None:
            col = tonemap_func(col)
        col[0, sel] = output["coarse_raycolor"][0]
    op = torch.zeros([B, OR, output["coarse_point_opacity"].shape[2]], dtype=torch.float32, device=dev)
    op[0, sel] = output["coarse_point_opacity"][0]
    qs = torch.ones([B, OR, 3], dtype=torch.float32, device=dev)
    qs[0, sel] = output["queried_shading"][0]
    out = dict(output)
    out.update(coarse_is_background=bgt, coarse_mask=1 - bgt, coarse_raycolor=col, coarse_point_opacity=op, queried_shading=qs)
    if prob == 1 and "ray_max_shading_opacity" in output:
        for k in PROBE_KEYS:
            if output.get(k) is not None:
                t = torch.zeros([B, OR, *output[k].shape[2:]], dtype=output[k].dtype, device=dev)
                t[0, sel] = output[k][0]
                out[k] = t
    dense_geometry = output.get("_dense_geometry")
    if isinstance(dense_geometry, tuple):      # the differentiable form of a ``geometry_grad`` step: for the loss, not a set of maps
        dense_geometry = None
    for k, name in GEOMETRY_KEYS:             # the depth and opacity maps of a ``ray_geometry`` render: 0 on the rays that missed
        if dense_geometry is not None:         # (ops.ray_geometry has written every ray's value, zeros for the misses: the scatter's result)
            out[k] = dense_geometry[name][None, :, None]
        elif output.get(k) is not None:
            t = torch.zeros([B, OR, *output[k].shape[2:]], dtype=output[k].dtype, device=dev)
            t[0, sel] = output[k][0]
            out[k] = t
    return out

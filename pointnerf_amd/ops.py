"""Thin host wrappers: torch tensors (device memory, streams) -> C-ABI calls of libpnerf_hip.so.

PyTorch is plumbing here: it owns HBM allocations and the stream; every computation on the hot
path happens inside the library.  All functions require CUDA(=HIP) tensors and raise otherwise.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return ctypes.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "pointnerf_amd ops need contiguous device tensors"
    return ctypes.c_void_p(t.data_ptr())


def host_array(t):
    """The small tensors of a step that the host needs as numbers (camera position / rotation, background, near / far, Rw2c: 3 .. 9 floats)
    as a numpy array.  A device tensor is read back ONCE per (tensor object, version): the copy is cached on the tensor object itself and is
    valid as long as the tensor's in-place version counter has not moved (a new tensor -- the reference's ``set_input`` makes one per batch --
    is read back again).  Every read-back is a host synchronisation with the device idle behind it: a step made eight of them (near, far,
    camera position twice, rotation, background, Rw2c, counters) where one is needed."""
    if not isinstance(t, torch.Tensor):
        return np.asarray(t)
    if not t.is_cuda:
        return t.detach().numpy()
    # Only step INPUTS are cached: a Parameter (Rw2c, when it is learnable) is written through .data / optimizer kernels without a version
    # bump, and an inference-mode tensor has no version counter at all (t._version raises): both are read back every time.
    cacheable = not isinstance(t, torch.nn.Parameter) and not t.requires_grad
    ver = None
    if cacheable:
        try:
            ver = t._version
        except Exception:
            cacheable = False
    if cacheable:
        c = getattr(t, "_pnerf_host", None)
        if c is not None and c[0] == ver and c[2] == t.data_ptr():      # (data_ptr: t.data = ... / set_() re-home a tensor without a version bump)
            return c[1]
    arr = t.detach().cpu().numpy()
    arr.setflags(write=False)                                            # callers share the cached copy
    if cacheable:
        try:
            t._pnerf_host = (ver, arr, t.data_ptr())
        except Exception:
            pass
    return arr


def _need_cuda(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("pointnerf_amd: %s must be a device tensor (this path has no CPU implementation)" % name)


def _dense_arg(t, name, dtype, numel=None):
    _need_cuda(t, name)
    if t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise ValueError("pointnerf_amd: %s must be a contiguous %s tensor%s, got %s %s"
                         % (name, dtype, "" if numel is None else " of %d elements" % numel, t.dtype, list(t.shape)))
    return t


def _dense_args(anchor_name, anchor, *specs):
    """_dense_arg on every (name, tensor, dtype, numel) of ``specs``, in their order; then, with an anchor, every tensor must be on the anchor's
    device (anchor_name = None: no device check)"""
    for name, t, dtype, numel in specs:
        _dense_arg(t, name, dtype, numel)
    if anchor_name is not None:
        for name, t, _, _ in specs:
            if t.device != anchor.device:
                raise ValueError("pointnerf_amd: %s is on %s, %s on %s" % (name, t.device, anchor_name, anchor.device))


def _render_outputs(R, SR, K, device):
    """the six results of a render forward, uninitialised: decoded, weight, ray_color, opacity, bg_trans, blend_w"""
    f32 = dict(dtype=torch.float32, device=device)
    return (torch.empty(R, SR, 4, **f32), torch.empty(R, SR, K, **f32), torch.empty(R, 3, **f32), torch.empty(R, SR, **f32),
            torch.empty(R, **f32), torch.empty(R, SR, **f32))


# ------------------------------------------------------------------------------------------ grid
def mid_depths(D, near, far):
    """The D mid-point depths of near_far_linear_ray_generation with jitter=0
    (models/rendering/diff_ray_marching.py:369-384), computed on the host with the same fp32 op
    sequence (linspace, lerp, diff, cumsum, midpoint) so that samples are bit-identical."""
    t = torch.linspace(0, 1, D + 1).view(1, -1)
    t = near * (1 - t) + far * t
    seg = (t[..., 1:] - t[..., :-1]) * (1 + 0.0 * (torch.zeros(1, 1, D) - 0.5))
    end = torch.cumsum(seg, dim=2)
    end = near + torch.cat([torch.zeros(1, 1, 1), end], dim=2)
    mid = (end[:, :, :-1] + end[:, :, 1:]) / 2
    return mid.reshape(-1).contiguous(), seg.reshape(-1).contiguous()


def grid_hyperparameters(opt, xyz):
    """lighting_fast_querier.get_hyperparameters (models/neural_points/point_query.py:47-71) and the
    constants of :35-42, read from ``opt`` at call time.  One device->host sync (the min/max),
    amortised by the grid cache."""
    vsize64 = np.asarray(opt.vsize, dtype=np.float64)
    vscale = np.asarray(opt.vscale, dtype=np.int32)
    scaled_vsize = (np.asarray(opt.vsize) * vscale).astype(np.float32)
    radius = np.asarray(opt.radius_limit_scale * max(opt.vsize[0], opt.vsize[1])).astype(np.float32)
    _need_cuda(xyz, "xyz")
    xyz = xyz.contiguous()
    mm6 = torch.empty(6, dtype=torch.float32, device=xyz.device)
    L.check(L.lib().pnerf_points_minmax(_ptr(xyz), int(xyz.shape[0]), _ptr(mm6), _stream()), "pnerf_points_minmax")
    mm = mm6.cpu().numpy().reshape(2, 3)                  # (the one device -> host read of a grid rebuild; fp32 arithmetic below, like the reference's torch ops)
    rmin = np.asarray(opt.ranges[:3], dtype=np.float32)
    rmax = np.asarray(opt.ranges[3:], dtype=np.float32)
    mn, mx = np.maximum(mm[0], rmin), np.minimum(mm[1], rmax)
    pad = (scaled_vsize * np.asarray(opt.kernel_size) / 2).astype(np.float32)
    mn, mx = (mn - pad).astype(np.float32), (mx + pad).astype(np.float32)
    vdim = (mx - mn).astype(np.float32) / vsize64
    scaled_vdim = np.ceil(vdim / vscale).astype(np.int32)
    ranges = np.concatenate([mn, mx]).astype(np.float32)
    return ranges, scaled_vsize, scaled_vdim, float(radius)


def make_grid_params(ranges, scaled_vsize, scaled_vdim, kernel_size, query_size, P, max_o, radius):
    gp = L.GridParams()
    gp.ranges[:] = [float(x) for x in ranges]
    gp.vsize[:] = [float(x) for x in scaled_vsize]
    gp.vdim[:] = [int(x) for x in scaled_vdim]
    gp.kernel_size[:] = [int(x) for x in kernel_size]
    gp.query_size[:] = [int(x) for x in query_size]
    gp.P, gp.max_o, gp.radius = int(P), int(max_o), float(radius)
    return gp


class VoxelGrid:
    """A built grid: params + the device workspace that holds it."""

    def __init__(self, gp, ws, n_points):
        self.gp, self.ws, self.n_points = gp, ws, n_points
        self._info = None

    def info(self):
        """dict(n_in_grid, n_occ, max_cnt, cell0, first_idx); synchronises the stream once."""
        if self._info is None:
            buf = (ctypes.c_int32 * L.GI_LEN)()
            L.check(L.lib().pnerf_grid_info(_ptr(self.ws), buf, _stream()), "pnerf_grid_info")
            self._info = dict(n_in_grid=buf[0], n_occ=buf[1], max_cnt=buf[2], cell0=buf[3], first_idx=buf[4],
                              overflow_max_o=buf[1] > self.gp.max_o, overflow_P=buf[2] > self.gp.P)
        return self._info


def build_grid(gp, xyz):
    """xyz [N,3] f32 device tensor -> VoxelGrid (enqueues only)."""
    _need_cuda(xyz, "xyz")
    xyz = xyz.detach().reshape(-1, 3).contiguous().float()
    n = xyz.shape[0]
    lib = L.lib()
    nbytes = lib.pnerf_grid_workspace_bytes(ctypes.byref(gp), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
    L.check(lib.pnerf_grid_build(ctypes.byref(gp), _ptr(xyz), n, _ptr(ws), nbytes, _stream()), "pnerf_grid_build")
    return VoxelGrid(gp, ws, n)


# ------------------------------------------------------------------------------------------ query
def query_dense(grid, R, D, SR, K, raypos=None, campos=None, raydir=None, mid=None, near=0.0, far=0.0,
                jitter=0.0, seed=0):
    """pnerf_query: dense-over-R outputs, no host sync.  Returns a dict of device tensors."""
    dev = grid.ws.device
    lib = L.lib()
    loc = torch.empty(R, SR, 3, dtype=torch.float32, device=dev)
    pidx = torch.empty(R, SR, K, dtype=torch.int32, device=dev)
    nn = torch.empty(R, SR, dtype=torch.int32, device=dev)
    hit = torch.empty(R, dtype=torch.int32, device=dev)
    vlist = torch.empty(max(R * SR, 1), dtype=torch.int32, device=dev)
    counters = torch.empty(8, dtype=torch.int32, device=dev)
    nws = lib.pnerf_query_workspace_bytes(R, SR)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    cam = None
    if raypos is None:
        cam = (ctypes.c_float * 3)(*[float(x) for x in campos])
        _need_cuda(raydir, "raydir"); _need_cuda(mid, "mid")
    L.check(lib.pnerf_query(ctypes.byref(grid.gp), _ptr(grid.ws), _ptr(raypos), cam, _ptr(raydir), _ptr(mid),
                            float(near), float(far), float(jitter), int(seed) & (2 ** 64 - 1), R, D, SR, K,
                            _ptr(loc), _ptr(pidx), _ptr(nn), _ptr(hit), _ptr(vlist), _ptr(counters),
                            _ptr(ws), nws, _stream()), "pnerf_query")
    return dict(sample_loc=loc, sample_pidx=pidx, sample_nn=nn, ray_hit=hit, valid_list=vlist, counters=counters)


def jitter_uniforms(seed, R, D, device):
    """The uniforms U[r, d] the jittered query draws for ``seed`` (pnerf_debug_uniform): [1, R, D] f32 device tensor."""
    out = torch.empty(1, R, D, dtype=torch.float32, device=device)
    L.check(L.lib().pnerf_debug_uniform(int(seed) & (2 ** 64 - 1), 0, R * D, _ptr(out), _stream()), "pnerf_debug_uniform")
    return out


# ------------------------------------------------------------------------------------------ MLP + renderer
def mlp_layout():
    """name -> (offset, shape) of the flat parameter vector, reference state_dict order."""
    offs = (ctypes.c_int64 * (L.MLP_NTENSORS + 1))()
    L.check(L.lib().pnerf_mlp_layout(32, offs), "pnerf_mlp_layout")
    names = ["block1.0", "block1.2", "block3.0", "block3.2", "alpha_branch.0",
             "color_branch.0", "color_branch.2", "color_branch.4", "color_branch.6"]
    shapes = [(256, 284), (256, 256), (256, 263), (256, 256), (1, 256), (128, 280), (128, 128), (128, 128), (3, 128)]
    out, i = {}, 0
    for n, shp in zip(names, shapes):
        out[n + ".weight"] = (offs[i], shp); out[n + ".bias"] = (offs[i + 1], (shp[0],)); i += 2
    return out, offs[L.MLP_NTENSORS]


def flatten_mlp(state, device):
    """dict of reference-named tensors -> flat fp32 device vector."""
    lay, total = mlp_layout()
    flat = torch.empty(total, dtype=torch.float32, device=device)
    for k, (o, shp) in lay.items():
        flat[o:o + int(np.prod(shp))] = state[k].detach().reshape(-1).to(device=device, dtype=torch.float32)
    return flat


def pack_mlp(flat, out=None):
    """Re-pack the flat parameters into MFMA fragment order (must be called after every weight update)."""
    _need_cuda(flat, "mlp parameters")
    lib = L.lib()
    if out is None:
        out = torch.empty(lib.pnerf_mlp_packed_bytes(), dtype=torch.uint8, device=flat.device)
    L.check(lib.pnerf_mlp_pack(_ptr(flat), _ptr(out), _stream()), "pnerf_mlp_pack")
    return out


def make_camera(campos, camrot, vsize_z, raydist_mode_unit=1, bg=None, rw2c=None):
    c = L.Camera()
    c.campos[:] = [float(x) for x in np.asarray(campos, dtype=np.float64).reshape(-1)[:3]]
    c.camrot[:] = [float(x) for x in np.asarray(camrot, dtype=np.float64).reshape(-1)[:9]]
    r = np.eye(3) if rw2c is None else np.asarray(rw2c, dtype=np.float64)
    c.rw2c[:] = [float(x) for x in r.reshape(-1)[:9]]
    c.vsize_z = float(vsize_z)
    c.raydist_mode_unit = int(raydist_mode_unit)
    if bg is None:
        c.has_bg = 0
        c.bg[:] = [0.0, 0.0, 0.0]
    else:
        c.has_bg = 1
        c.bg[:] = [float(x) for x in np.asarray(bg, dtype=np.float64).reshape(-1)[:3]]
    return c


def frames_table(Rw2c, n_points):
    """The [N,9] device view of a per-point Rw2c table [N,3,3] that pnerf_points.frames takes (no copy for a contiguous fp32 table; never a
    host copy: the table is 72 MB at 2 M points).  Also refuses the arithmetic settings no FRAMES kernel instance exists for."""
    _need_cuda(Rw2c, "Rw2c")
    if Rw2c.dim() != 3 or tuple(Rw2c.shape) != (int(n_points), 3, 3):
        raise ValueError("pointnerf_amd: per-point Rw2c must be [%d, 3, 3], got %s" % (int(n_points), list(Rw2c.shape)))
    if arithmetic()[0] != 3:
        raise NotImplementedError("pointnerf_amd: per-point Rw2c is not implemented for set_inference_products(2) (pnerf_set_inference_products); "
                                  "set it back to 3")
    if cross_terms_state()[1] & 1:
        raise NotImplementedError("pointnerf_amd: per-point Rw2c is not implemented for e4m3 cross terms in the inference forward (bit 0 of "
                                  "set_cross_terms(8, where), pnerf_set_cross_terms_where); clear the bit")
    return Rw2c.detach().reshape(-1, 9).contiguous().float()


def make_points(xyz, emb, conf, pdir, color, frames=None):
    """``frames``: optional [N,9] fp32 device table of per-point Rw2c frames (frames_table); the returned structure keeps it alive."""
    for n, t in (("xyz", xyz), ("points_embeding", emb), ("points_conf", conf), ("points_dir", pdir), ("points_color", color)):
        _need_cuda(t, n)
        assert t.is_contiguous() and t.dtype == torch.float32, n
    p = L.Points()
    p.xyz, p.embedding, p.conf, p.dir, p.color = xyz.data_ptr(), emb.data_ptr(), conf.data_ptr(), pdir.data_ptr(), color.data_ptr()
    p.n, p.feat_dim = int(xyz.reshape(-1, 3).shape[0]), int(emb.shape[-1])
    if frames is not None:
        _need_cuda(frames, "Rw2c frames")
        assert frames.is_contiguous() and frames.dtype == torch.float32 and tuple(frames.shape) == (p.n, 9), "frames"
        p.frames, p._frames_keep = frames.data_ptr(), frames
    return p


def frames_are_render_only(frames, train, hint=""):
    """THE refusal of per-point Rw2c frames in a training forward (and so in any backward): pnerf_points.frames is render-only."""
    if frames is not None and train:
        raise NotImplementedError("per-point Rw2c (scene editing) is render-only: run the forward under torch.no_grad() -- the reference "
                                  "freezes Rw2c and editing never trains" + hint)


def make_step(raydir, dense, flat, packed, R, SR, K, n_valid, xyz_pers=None, loc_pers=None):
    """pnerf_step: the inputs the four render entry points share.  ``dense`` = the query's dict (sample_loc, sample_pidx, valid_list, counters and,
    for the render pair, sample_nn); ``n_valid`` = the capacity in valid samples (>= counters[0]; the same for the forward and the backward of a
    step); ``xyz_pers`` / ``loc_pers`` (both or neither) for the stand-alone aggregator.  The returned structure keeps the tensors it points into alive."""
    R, SR, K = int(R), int(SR), int(K)
    f32, i32 = torch.float32, torch.int32
    fields = [("raydir", raydir, f32, R * 3), ("sample_loc", dense["sample_loc"], f32, R * SR * 3), ("sample_pidx", dense["sample_pidx"], i32, R * SR * K),
              ("valid_list", dense["valid_list"], i32, None), ("counters", dense["counters"], i32, 8), ("params", flat, f32, None),
              ("packed_mlp", packed, torch.uint8, None)]
    fields += [f for f in (("sample_nn", dense.get("sample_nn"), i32, R * SR), ("xyz_pers", xyz_pers, f32, None), ("loc_pers", loc_pers, f32, R * SR * 3))
               if f[1] is not None]                     # (half a pair of perspective coordinates: the library's PNERF_E_INVAL)
    st = L.Step()
    for name, t, dtype, numel in fields:
        setattr(st, name, _ptr(_dense_arg(t, name, dtype, numel)))
    st.R, st.SR, st.K, st.n_valid_max = R, SR, K, int(n_valid)
    st._keep = [t for _, t, _, _ in fields]
    return st


def _forward_scratch(n_valid, K, train, device):
    """what a forward works in, (saved, ws, ws_bytes): an arena block of pnerf_agg_saved_bytes (training; handed back with ARENA.give) or a
    workspace of pnerf_agg_workspace_bytes (inference)"""
    lib = L.lib()
    if train:
        return ARENA.take(lib.pnerf_agg_saved_bytes(n_valid, K), device), None, 0
    nws = lib.pnerf_agg_workspace_bytes(n_valid, K)
    return None, torch.empty(nws, dtype=torch.uint8, device=device), nws


def _point_grads(grads, ready_event=None, zero_one=None):
    """pnerf_point_grads over grads = dict(points_embeding, points_conf, points_dir, points_color[, xyz]) (device tensors, added to)"""
    pg = L.PointGrads()
    pg.embedding, pg.conf = grads["points_embeding"].data_ptr(), grads["points_conf"].data_ptr()
    pg.dir, pg.color = grads["points_dir"].data_ptr(), grads["points_color"].data_ptr()
    if grads.get("xyz") is not None:
        pg.xyz = grads["xyz"].data_ptr()
    if zero_one is not None:
        pg.zero_one_gscale, pg.zero_one_eps = zero_one[0].data_ptr(), float(zero_one[1])
    if ready_event is not None:          # a torch.cuda.Event that has been recorded once (so that its hipEvent_t exists)
        pg.ready_event = ready_event.cuda_event
    return pg


class Arena:
    """Grow-only device scratch for the saved activations of one in-flight training forward.  The arena is tens of GB
    at bench size and its exact size changes every step with the number of valid samples; letting torch's caching
    allocator see a new size each step costs a hipMalloc/hipFree pair of that size (measured: ~1.9 s per step)."""

    def __init__(self):
        self.free, self.headroom = [], 1.15

    def take(self, nbytes, device):
        best = None
        for t in self.free:
            if t.numel() >= nbytes and t.device == device and (best is None or t.numel() < best.numel()):
                best = t
        if best is not None:
            self.free.remove(best)
            return best
        self.free = [t for t in self.free if t.device != device]      # drop too-small blocks before growing
        return torch.empty(int(nbytes * self.headroom) + 256, dtype=torch.uint8, device=device)

    def give(self, t):
        if t is not None:
            self.free.append(t)

    def capacity_samples(self, K, device):
        """the number of valid samples the largest free block can hold the saved activations of (0: no free block yet): the capacity a
        render step can be ENQUEUED with before the step's own count has reached the host (NeuralPointsRayMarching.render_dense)"""
        best = max((t.numel() for t in self.free if t.device == torch.device(device)), default=0)
        if best <= 0:
            return 0
        key = (best, int(K))
        hit = getattr(self, "_cap_cache", {}).get(key)
        if hit is not None:
            return hit
        fn = L.lib().pnerf_agg_saved_bytes
        lo, hi = 0, best // 512
        while lo < hi:                          # largest n with saved_bytes(n, K) <= best (monotone)
            mid = (lo + hi + 1) // 2
            if fn(mid, int(K)) <= best:
                lo = mid
            else:
                hi = mid - 1
        self._cap_cache = {key: lo}
        return lo

    def reserve(self, nbytes, device):
        """make sure one free block of at least ``nbytes`` exists (a caller that knows its largest step sizes the arena once,
        instead of paying a ~2 s hipFree + hipMalloc of tens of GB when a later step is 15 % larger than every earlier one)"""
        if not any(t.numel() >= nbytes and t.device == device for t in self.free):
            self.give(self.take(nbytes, device))


ARENA = Arena()


def arena_budget_bytes():
    """Upper bound for the saved-activation arena of ONE render step (5.9 KB per neighbor row incl. the per-sample areas: 44 GB at the bench configuration).
    A training step whose rows would need more (Barn-scale clouds at K = 12, large ray batches) does not fail or swap: its forward runs
    in inference mode and its backward re-runs the forward chunk of rays by chunk of rays, each chunk within the budget
    (fused.FusedRender).  PNERF_ARENA_BUDGET_GB overrides the default of 160 GB (of the 288 GB of an MI355X)."""
    import os
    return int(float(os.environ.get("PNERF_ARENA_BUDGET_GB", "160")) * (1 << 30))


def compact_valid(sample_nn):
    """work list of the samples with neighbors: (valid_list [n] i32, counters [8] i32) from sample_nn [R,SR] (pnerf_compact_valid)"""
    lib = L.lib()
    n = sample_nn.numel()
    dev = sample_nn.device
    vlist = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counters = torch.empty(8, dtype=torch.int32, device=dev)
    nws = lib.pnerf_compact_workspace_bytes(n)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    L.check(lib.pnerf_compact_valid(_ptr(sample_nn), n, _ptr(vlist), _ptr(counters), _ptr(ws), nws, _stream()), "pnerf_compact_valid")
    return vlist, counters


def touched_flags(pidx, n_points):
    """[n_points] int32 0/1 flags of the points that occur in the int32 neighbor table ``pidx`` (row 0 also when a slot is empty):
    pnerf_touched_flags, one pass over the table, no int64 temporaries"""
    _need_cuda(pidx, "pidx")
    if pidx.dtype != torch.int32 or not pidx.is_contiguous():
        raise ValueError("touched_flags: a contiguous int32 neighbor table is expected")
    flags = torch.empty(max(int(n_points), 0), dtype=torch.int32, device=pidx.device)
    L.check(L.lib().pnerf_touched_flags(_ptr(pidx), pidx.numel(), int(n_points), _ptr(flags), _stream()), "pnerf_touched_flags")
    return flags


def reserve_pool(nbytes, device):
    """Pre-size torch's caching allocator for the step's variable-size tensors (everything indexed by the number of rays
    that hit the cloud: compacted weights / indices / confidences, the loss temporaries and their gradients).  Their sizes
    change with every batch, so without a pool the allocator keeps meeting requests no cached block fits and calls
    hipMalloc in the middle of training steps (measured: 3 per step, each a device-wide stall, 15 ms per step on a
    freshly booted box).  One block of the worst-case size, allocated and released once, is split and re-merged by the
    allocator from then on."""
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    del t


def render_forward(cam, pts, packed, flat, raydir, dense, R, SR, K, n_valid, train):
    """pnerf_render_forward.  n_valid = host copy of dense['counters'][0] (capacity of the scratch).
    Returns dict(decoded, weight, ray_color, opacity, bg_trans, blend_w, saved)."""
    dev = raydir.device
    decoded, weight, ray_color, opacity, bg_trans, blend_w = _render_outputs(R, SR, K, dev)
    st = make_step(raydir, dense, flat, packed, R, SR, K, n_valid)
    saved, ws, nws = _forward_scratch(n_valid, K, train, dev)
    L.check(L.lib().pnerf_render_forward(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st),
                                         _ptr(decoded), _ptr(weight), _ptr(ray_color), _ptr(opacity), _ptr(bg_trans), _ptr(blend_w),
                                         _ptr(saved), _ptr(ws), nws, _stream()), "pnerf_render_forward")
    return dict(decoded=decoded, weight=weight, ray_color=ray_color, opacity=opacity, bg_trans=bg_trans,
                blend_w=blend_w, saved=saved)


def check_cutoff(cutoff, stage):
    """(cutoff, stage) of a cut render as numbers, refusing what pnerf_render_forward_cut refuses: a transmittance cutoff outside [0, 1), a
    stage of less than one sample"""
    cutoff, stage = float(cutoff), int(stage)
    if not (0.0 <= cutoff < 1.0):
        raise ValueError("pointnerf_amd: transmittance_cutoff must lie in [0, 1), got %r" % (cutoff,))
    if stage < 1:
        raise ValueError("pointnerf_amd: cutoff_stage must be at least 1, got %r" % (stage,))
    return cutoff, stage


def render_forward_cut(cam, pts, packed, flat, raydir, dense, R, SR, K, n_valid, cutoff, stage):
    """pnerf_render_forward_cut: the render-only forward with early ray termination -- rays are shaded front to back in stages of ``stage``
    sample slots and leave once their transmittance is below ``cutoff`` (include/pnerf.h; the reference has no counterpart, the transmittance
    is ray_march's, models/rendering/diff_ray_marching.py:508-554).  Returns render_forward's dict (saved = None; samples that were not
    shaded are 0 in decoded / weight / opacity / blend_w, bg_trans of a cut ray is its transmittance at termination) plus ``cut_counters``,
    a [4] int32 device tensor: samples shaded, rays that ended with a valid sample unshaded, 0, 0.  No host read."""
    cutoff, stage = check_cutoff(cutoff, stage)
    lib = L.lib()
    dev = raydir.device
    decoded, weight, ray_color, opacity, bg_trans, blend_w = _render_outputs(R, SR, K, dev)
    cut_counters = torch.empty(4, dtype=torch.int32, device=dev)
    st = make_step(raydir, dense, flat, packed, R, SR, K, n_valid)
    _, ws, nws = _forward_scratch(n_valid, K, False, dev)
    ncut = lib.pnerf_render_cut_workspace_bytes(R, SR) if cutoff > 0 else 0
    cut_ws = torch.empty(ncut, dtype=torch.uint8, device=dev) if ncut else None
    L.check(lib.pnerf_render_forward_cut(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), cutoff, stage,
                                         _ptr(decoded), _ptr(weight), _ptr(ray_color), _ptr(opacity), _ptr(bg_trans), _ptr(blend_w),
                                         _ptr(cut_counters), _ptr(ws), nws, _ptr(cut_ws), ncut, _stream()), "pnerf_render_forward_cut")
    return dict(decoded=decoded, weight=weight, ray_color=ray_color, opacity=opacity, bg_trans=bg_trans, blend_w=blend_w, saved=None,
                cut_counters=cut_counters)


def cut_stage(cam, sample_loc, sample_nn, ray_hit, decoded, cutoff, stage_samples, stage, state=None):
    """pnerf_cut_stage: one stage of the cut render on dense arrays (sample_loc [R,SR,3], sample_nn [R,SR] i32, ray_hit [R] i32, decoded
    [R,SR,4] as the earlier stages left it).  ``state`` = the dict a previous stage returned (None for stage 0); returns
    dict(trans [R], depth_max [R], alive [R] i32 -- the per-ray state, updated in place --, flags [R,SR] i32, list, counters [8] i32)."""
    R, SR = int(sample_nn.shape[0]), int(sample_nn.shape[1])
    f32, i32 = torch.float32, torch.int32
    _dense_args(None, None, ("sample_loc", sample_loc, f32, R * SR * 3), ("sample_nn", sample_nn, i32, R * SR), ("ray_hit", ray_hit, i32, R),
                ("decoded", decoded, f32, R * SR * 4))
    dev = sample_nn.device
    if state is None:
        state = dict(trans=torch.empty(R, dtype=f32, device=dev), depth_max=torch.empty(R, dtype=f32, device=dev), alive=torch.empty(R, dtype=i32, device=dev))
    out = dict(trans=state["trans"], depth_max=state["depth_max"], alive=state["alive"], flags=torch.empty(R, SR, dtype=i32, device=dev),
               list=torch.empty(max(R * SR, 1), dtype=i32, device=dev), counters=torch.empty(8, dtype=i32, device=dev))
    lib = L.lib()
    nws = lib.pnerf_compact_workspace_bytes(R * SR)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    L.check(lib.pnerf_cut_stage(ctypes.byref(cam), _ptr(sample_loc), _ptr(sample_nn), _ptr(ray_hit), _ptr(decoded), R, SR, float(cutoff), int(stage_samples),
                                int(stage), _ptr(out["trans"]), _ptr(out["depth_max"]), _ptr(out["alive"]), _ptr(out["flags"]), _ptr(out["list"]),
                                _ptr(out["counters"]), _ptr(ws), nws, _stream()), "pnerf_cut_stage")
    return out


def render_backward(cam, pts, packed, flat, raydir, dense, R, SR, K, n_valid, fwd, grad_ray_color, grad_flat, grads, ready_event=None, zero_one=None,
                    grad_geom=None):
    """pnerf_render_backward: accumulates into grad_flat (MLP) and grads = dict(points_embeding=..., points_conf=...,
    points_dir=..., points_color=...) (device tensors, same shapes as the parameters); an ``xyz`` entry ([N,3] or [1,N,3]) receives d xyz
    (xyz_grad: pnerf_point_grads.xyz), without it none is formed.  ``zero_one`` = (scale [1] f32 device tensor, eps): the
    conf gradient of the zero-one regulariser over the hit rays' neighbor table is added by the same call (pnerf_point_grads.zero_one_gscale;
    ``dense`` must be the query's own output: its counters [1] and [3] count the empty slots).  ``grad_geom`` [R,3] f32 = the per-ray gradients
    with respect to (depth_sum, acc, bg_trans) (geometry_grad): pnerf_render_backward_geom; None: pnerf_render_backward itself."""
    lib = L.lib()
    st = make_step(raydir, dense, flat, packed, R, SR, K, n_valid)
    pg = _point_grads(grads, ready_event, zero_one)
    nws = lib.pnerf_render_backward_workspace_bytes(R, SR)
    ws = torch.empty(nws, dtype=torch.uint8, device=raydir.device)
    g = grad_ray_color.contiguous().float()
    if grad_geom is None:
        L.check(lib.pnerf_render_backward(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), _ptr(fwd["decoded"]), _ptr(fwd["weight"]), _ptr(g),
                                          _ptr(fwd["saved"]), _ptr(grad_flat), ctypes.byref(pg), _ptr(ws), nws, _stream()), "pnerf_render_backward")
        return
    gg = _dense_arg(grad_geom.contiguous().float(), "grad_geom", torch.float32, 3 * R)
    L.check(lib.pnerf_render_backward_geom(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), _ptr(fwd["decoded"]), _ptr(fwd["weight"]), _ptr(g), _ptr(gg),
                                           _ptr(fwd["saved"]), _ptr(grad_flat), ctypes.byref(pg), _ptr(ws), nws, _stream()), "pnerf_render_backward_geom")


def agg_forward(cam, pts, st, train):
    """pnerf_agg_forward on ``st`` = make_step(...) of the gathered per-slot arrays (no sample_nn; xyz_pers / loc_pers optional).
    Returns dict(decoded [R,SR,4], weight [R,SR,K], saved)."""
    f32 = dict(dtype=torch.float32, device=st._keep[0].device)
    decoded, weight = torch.empty(st.R, st.SR, 4, **f32), torch.empty(st.R, st.SR, st.K, **f32)
    saved, ws, nws = _forward_scratch(st.n_valid_max, st.K, train, f32["device"])
    L.check(L.lib().pnerf_agg_forward(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), _ptr(decoded), _ptr(weight),
                                      _ptr(saved), _ptr(ws), nws, _stream()), "pnerf_agg_forward")
    return dict(decoded=decoded, weight=weight, saved=saved)


def agg_backward(cam, pts, st, fwd, grad_decoded, grad_flat, grads):
    """pnerf_agg_backward for its forward's ``st`` and result ``fwd``: accumulates into grad_flat (MLP) and the per-slot ``grads`` (the keys of
    render_backward's)."""
    lib = L.lib()
    pg = _point_grads(grads)
    nws = lib.pnerf_render_backward_workspace_bytes(0, 1)      # (no [R,SR,4] gradient of its own: the weight-gradient partials only)
    ws = torch.empty(nws, dtype=torch.uint8, device=grad_flat.device)
    gd = grad_decoded.reshape(st.R, st.SR, 4).contiguous().float()
    L.check(lib.pnerf_agg_backward(ctypes.byref(cam), ctypes.byref(pts), ctypes.byref(st), _ptr(fwd["decoded"]), _ptr(fwd["weight"]), _ptr(gd),
                                   _ptr(fwd["saved"]), _ptr(grad_flat), ctypes.byref(pg), _ptr(ws), nws, _stream()), "pnerf_agg_backward")


# ------------------------------------------------------------------------------------------ gather (autograd)
class GatherRows(torch.autograd.Function):
    """rows = src[max(idx, 0)]  (NeuralPoints.forward's index_select, neural_points.py:706-717) with the
    scatter-add backward, both in libpnerf_hip.so.  src [N,W] f32, idx [...] i32 -> [..., W]."""

    @staticmethod
    def forward(ctx, src, idx):
        _need_cuda(src, "src")
        s2 = src.detach().reshape(-1, src.shape[-1]).contiguous().float()
        i2 = idx.reshape(-1).contiguous().to(torch.int32)
        out = torch.empty(i2.numel(), s2.shape[1], dtype=torch.float32, device=src.device)
        L.check(L.lib().pnerf_gather_rows(_ptr(s2), s2.shape[0], s2.shape[1], _ptr(i2), i2.numel(), _ptr(out), _stream()),
                "pnerf_gather_rows")
        ctx.save_for_backward(i2)
        ctx.src_shape = tuple(src.shape)
        return out.view(tuple(idx.shape) + (s2.shape[1],))

    @staticmethod
    def backward(ctx, g):
        (i2,) = ctx.saved_tensors
        w = ctx.src_shape[-1]
        gs = torch.zeros(ctx.src_shape, dtype=torch.float32, device=g.device)
        g2 = g.reshape(-1, w).contiguous().float()
        n_src = gs.numel() // w
        L.check(L.lib().pnerf_scatter_add_rows(_ptr(g2), _ptr(i2), i2.numel(), w, _ptr(gs), n_src, _stream()),
                "pnerf_scatter_add_rows")
        return gs, None


def gather_rows(src, idx):
    return GatherRows.apply(src, idx)


def zero_one_sum(conf_flat, pidx, ray_hit, eps):
    """The regulariser's forward pass: sum over the neighbor slots of  log(v) + log(1 - v),  v = clamp(gradient_clamp(conf[max(pidx, 0)], 1e-4, 1),
    eps, 1 - eps), as a scalar tensor (the per-block partial sums, added).  ``ray_hit`` None: every slot of the flat index list ``pidx``
    (pnerf_zero_one_forward); else ``pidx`` is the DENSE neighbor table [R, ...] of a query and only the rays with ray_hit > 0 count
    (pnerf_zero_one_forward_rays: no [R'', SR, K] copy of the table is made)."""
    lib = L.lib()
    R = 0 if ray_hit is None else int(pidx.shape[0])
    # the one rule for the number of partial sums: a workgroup per 256 slots of the flat list / per ray of the table, at most 2048
    part = torch.empty(lib.pnerf_zero_one_blocks(pidx.numel() if ray_hit is None else R * 256), dtype=torch.float32, device=conf_flat.device)
    if ray_hit is None:
        L.check(lib.pnerf_zero_one_forward(_ptr(conf_flat), conf_flat.numel(), _ptr(pidx), pidx.numel(), float(eps), _ptr(part), _stream()), "pnerf_zero_one_forward")
    else:
        L.check(lib.pnerf_zero_one_forward_rays(_ptr(conf_flat), conf_flat.numel(), _ptr(pidx), _ptr(ray_hit), R, int(pidx.numel() // max(R, 1)), float(eps),
                                                _ptr(part), _stream()), "pnerf_zero_one_forward_rays")
    return part.sum()


def zero_one_add_grad(conf_flat, pidx, ray_hit, eps, gscale, grad_conf_flat):
    """The regulariser's backward pass: grad_conf_flat[max(pidx, 0)] += gscale[0] (1 / v - 1 / (1 - v)) where the clamp to [eps, 1 - eps] was
    inactive (``gscale`` a [1] f32 device tensor; the forms of ``zero_one_sum``)."""
    if ray_hit is None:
        L.check(L.lib().pnerf_zero_one_backward(_ptr(conf_flat), conf_flat.numel(), _ptr(pidx), pidx.numel(), float(eps), _ptr(gscale), _ptr(grad_conf_flat),
                                                _stream()), "pnerf_zero_one_backward")
    else:
        R = int(pidx.shape[0])
        L.check(L.lib().pnerf_zero_one_backward_rays(_ptr(conf_flat), conf_flat.numel(), _ptr(pidx), _ptr(ray_hit), R, int(pidx.numel() // max(R, 1)), float(eps),
                                                     _ptr(gscale), _ptr(grad_conf_flat), _stream()), "pnerf_zero_one_backward_rays")


class ZeroOneConf(torch.autograd.Function):
    """zero_one_sum / zero_one_add_grad as a differentiable function of points_conf: the numerator of the reference's ``loss_zero_one`` on
    ``conf_coefficient`` (models/base_rendering_model.py:630-641) without materialising the [R'', SR, K] tensor -- one HIP pass forward, one backward."""

    @staticmethod
    def forward(ctx, conf, pidx, ray_hit, eps):
        c = conf.detach().reshape(-1)
        _need_cuda(c, "points_conf")
        ctx.save_for_backward(c, pidx, ray_hit)
        ctx.eps, ctx.shape = float(eps), conf.shape
        return zero_one_sum(c, pidx, ray_hit, eps)

    @staticmethod
    def backward(ctx, g):
        c, pidx, ray_hit = ctx.saved_tensors
        grad = torch.zeros_like(c)
        zero_one_add_grad(c, pidx, ray_hit, ctx.eps, g.detach().reshape(1).to(torch.float32).contiguous(), grad)
        return grad.view(ctx.shape), None, None, None


def zero_one_conf_sum(conf, pidx, eps):
    return ZeroOneConf.apply(conf, pidx.contiguous().reshape(-1), None, eps)


def zero_one_conf_sum_rays(conf, pidx_dense, ray_hit, eps):
    return ZeroOneConf.apply(conf, pidx_dense.contiguous(), ray_hit.contiguous(), eps)


class ColorLossRays(torch.autograd.Function):
    """sum over the rays that hit of (colour - gt)^2 on the DENSE ray colours [R,3] (pnerf_color_loss_forward_rays / _backward_rays): the
    colour term of the training loss without the hit rays' compaction (argsort + index_selects + their scatter-back in the backward)."""

    @staticmethod
    def forward(ctx, ray_color, gt, ray_hit):
        _need_cuda(ray_color, "ray_color")
        lib = L.lib()
        c, g = ray_color.detach().reshape(-1, 3).contiguous().float(), gt.detach().reshape(-1, 3).contiguous().float()
        R = c.shape[0]
        part = torch.empty(lib.pnerf_color_loss_blocks(R), dtype=torch.float32, device=c.device)
        L.check(lib.pnerf_color_loss_forward_rays(_ptr(c), _ptr(g), _ptr(ray_hit), R, _ptr(part), _stream()), "pnerf_color_loss_forward_rays")
        ctx.save_for_backward(c, g, ray_hit)
        ctx.shape = ray_color.shape
        return part.sum()

    @staticmethod
    def backward(ctx, gout):
        c, g, ray_hit = ctx.saved_tensors
        grad = torch.empty_like(c)
        gs = gout.detach().reshape(1).to(torch.float32).contiguous()
        L.check(L.lib().pnerf_color_loss_backward_rays(_ptr(c), _ptr(g), _ptr(ray_hit), c.shape[0], _ptr(gs), _ptr(grad), _stream()),
                "pnerf_color_loss_backward_rays")
        return grad.view(ctx.shape), None, None


def color_loss_sum_rays(ray_color, gt, ray_hit):
    return ColorLossRays.apply(ray_color, gt, ray_hit.contiguous())


class GeometryLossRays(torch.autograd.Function):
    """(sum_r m^2 (d - gt_depth)^2, sum_r (1 - m)^2 (T - 1)^2) over the DENSE per-ray geometry of a geometry_grad render: depth_sum, acc and
    bg_trans [R] (the differentiable outputs of the render node), the rays' hit flags, gt_depth / gt_mask [R]; m = gt_mask, d = depth_sum /
    (acc + 1e-6), a ray that missed counts with d = 0 and T = 1 (pnerf_geometry_loss_forward_rays / _backward_rays: one pass forward, one
    backward).  The numerators of the reference's depth and bg loss items (models/base_rendering_model.py:610-626); the caller divides by its
    global ray count.  The backward hands (g_ds, g_acc, g_T) to the three inputs, the columns of ONE [R,3] tensor -- FusedRender.backward
    puts them back together for pnerf_render_backward_geom."""

    @staticmethod
    def forward(ctx, depth_sum, acc, bg_trans, ray_hit, gt_depth, gt_mask):
        _need_cuda(depth_sum, "depth_sum")
        lib = L.lib()
        R = int(ray_hit.numel())
        f32 = torch.float32
        flat = lambda t: t.detach().reshape(-1).contiguous().float()
        a = (flat(depth_sum), flat(acc), flat(bg_trans), ray_hit.reshape(-1).contiguous(), flat(gt_depth), flat(gt_mask))
        _dense_args("ray_hit", a[3], ("depth_sum", a[0], f32, R), ("acc", a[1], f32, R), ("bg_trans", a[2], f32, R), ("ray_hit", a[3], torch.int32, R),
                    ("gt_depth", a[4], f32, R), ("gt_mask", a[5], f32, R))
        nb = lib.pnerf_color_loss_blocks(R)
        part = torch.empty(2, nb, dtype=f32, device=a[0].device)
        L.check(lib.pnerf_geometry_loss_forward_rays(*[_ptr(t) for t in a], R, _ptr(part), _stream()), "pnerf_geometry_loss_forward_rays")
        ctx.save_for_backward(*a)
        ctx.shapes = (depth_sum.shape, acc.shape, bg_trans.shape)
        sums = part.sum(dim=1)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g_depth, g_bg):
        a = ctx.saved_tensors
        R = int(a[3].numel())
        dev = a[0].device
        gs = torch.stack([torch.zeros((), device=dev) if g is None else g.detach().reshape(()).to(torch.float32) for g in (g_depth, g_bg)]).contiguous()
        grad = torch.empty(R, 3, dtype=torch.float32, device=dev)
        L.check(L.lib().pnerf_geometry_loss_backward_rays(*[_ptr(t) for t in a], R, _ptr(gs), _ptr(grad), _stream()), "pnerf_geometry_loss_backward_rays")
        return grad[:, 0].reshape(ctx.shapes[0]), grad[:, 1].reshape(ctx.shapes[1]), grad[:, 2].reshape(ctx.shapes[2]), None, None, None


def geometry_loss_sums_rays(depth_sum, acc, bg_trans, ray_hit, gt_depth, gt_mask):
    return GeometryLossRays.apply(depth_sum, acc, bg_trans, ray_hit, gt_depth, gt_mask)


def set_inference_products(n):
    """Products per multiply-add of the inference forward: 3 (default, fp32-class accuracy, what the training forward always runs) or
    2 (render / evaluation option: ~1.5x less matrix work, ray colour within ~2e-5 of fp32).  Returns the previous setting."""
    old = L.lib().pnerf_set_inference_products(int(n))
    if old < 0:
        raise ValueError("inference products must be 2 or 3")
    return old


def set_wgrad_planes(n):
    """f16 planes per operand of the weight-gradient GEMMs of the training backward: 1 (default: one plane rounded to nearest, one MFMA
    product) or 2 (both operands as two planes, three products: fp32-class weight gradients, the reference arithmetic of the convergence
    A/B in tests/test_gpu_zz_convergence.py; twice the saved / streamed bytes).  Process-wide; choose it between steps, never between a
    training forward and its backward.  Returns the previous setting."""
    old = L.lib().pnerf_set_wgrad_planes(int(n))
    if old < 0:
        raise ValueError("weight-gradient planes must be 1 or 2")
    ARENA._cap_cache = {}                 # pnerf_agg_saved_bytes depends on the mode: a capacity cached under the other mode is off by ~2x
    return old


def set_cross_terms(bits, where=None):
    """Arithmetic of the cross terms h*m + m*h of the aggregator's tile GEMMs (csrc/mixq.h): 8 = e4m3 factors (default), 16 = f16 factors (csrc/f16x3.h,
    rounds 2-5).  `where` (optional) = which kernels use the e4m3 form: bit 0 inference forward, bit 1 training forward, bit 2 backward (default 4).
    Returns (previous bits, previous mask)."""
    old = L.lib().pnerf_set_cross_terms(int(bits))
    if old < 0:
        raise ValueError("cross terms must be 8 or 16")
    oldw = L.lib().pnerf_set_cross_terms_where(int(where)) if where is not None else None
    if where is not None and oldw < 0:
        raise ValueError("cross-term mask must be 0..7")
    return old, oldw


def set_tile_grid(max_workgroups=0):
    """Tests: cap the grid of the tile and colour kernels at `max_workgroups` (0: the default, as many workgroups as stay resident); which workgroup
    runs a tile changes no forward result, and gradients only by the order of their atomic additions (pnerf_debug_set_tile_grid).  Returns the
    previous cap."""
    old = L.lib().pnerf_debug_set_tile_grid(int(max_workgroups))
    if old < 0:
        raise ValueError("the grid cap must be >= 0")
    return old


def arithmetic():
    """(inference products, weight-gradient planes, cross-term bits, cross-term mask as stored): the process-wide settings of
    set_inference_products / set_wgrad_planes / set_cross_terms, read without writing (pnerf_get_arithmetic)."""
    out = (ctypes.c_int32 * 4)()
    L.check(L.lib().pnerf_get_arithmetic(out), "pnerf_get_arithmetic")
    return tuple(int(v) for v in out)


def cross_terms_state():
    """(bits, mask) in effect: see set_cross_terms (the mask counts only while the bits are 8)"""
    _, _, bits, mask = arithmetic()
    return bits, (mask if bits == 8 else 0)


# ------------------------------------------------------------------------------------------ evaluation scores
def image_metrics_sums(img, gt, win=11, data_range=2.0, quantize8=True):
    """pnerf_image_metrics on two [H, W, 3] float32 contiguous device images: float64 device tensor [sum of squared differences,
    SSIM-map sum of channel 0, 1, 2 over the (H - win + 1) x (W - win + 1) windows inside the image].  Enqueues only (no host read).
    Anything that is not exactly that layout raises: a float64 image or an [H, W, 4] one would otherwise be read as something else."""
    for name, t in (("img", img), ("gt", gt)):
        _need_cuda(t, name)
        if t.dtype != torch.float32:
            raise TypeError("pointnerf_amd: image_metrics needs float32 images, %s is %s" % (name, t.dtype))
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError("pointnerf_amd: image_metrics needs [H, W, 3] images, %s is %s" % (name, list(t.shape)))
        if not t.is_contiguous():
            raise ValueError("pointnerf_amd: image_metrics needs contiguous images, %s has strides %s" % (name, list(t.stride())))
    if img.shape != gt.shape or img.device != gt.device:
        raise ValueError("pointnerf_amd: image_metrics: img %s on %s and gt %s on %s differ" % (list(img.shape), img.device, list(gt.shape), gt.device))
    H, W = int(img.shape[0]), int(img.shape[1])
    lib = L.lib()
    nbytes = lib.pnerf_image_metrics_workspace_bytes(H, W, int(win))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=img.device)
    out4 = torch.empty(4, dtype=torch.float64, device=img.device)
    L.check(lib.pnerf_image_metrics(_ptr(img.detach()), _ptr(gt.detach()), H, W, int(win), float(data_range), 1 if quantize8 else 0,
                                    _ptr(out4), _ptr(ws), nbytes, _stream()), "pnerf_image_metrics")
    return out4


def image_metrics(img, gt, win=11, data_range=2.0, quantize8=True):
    """float64 device tensor [mse, ssim] of two [H, W, 3] float32 device images the way run/evaluate.py scores them (compare_ssim(gt, img,
    11, multichannel=True) of skimage <= 0.18 on float images: data_range 2; quantize8: through the 8-bit PNG round trip first).  No host
    read: the two divisions by the element / window counts are device operations on the kernel's sums."""
    out4 = image_metrics_sums(img, gt, win, data_range, quantize8)
    H, W = int(img.shape[0]), int(img.shape[1])
    n_win = (H - int(win) + 1) * (W - int(win) + 1)
    return torch.stack([out4[0] / float(H * W * 3), out4[1:].sum() / float(3 * n_win)])


# ------------------------------------------------------------------------------------------ depth maps from images (csrc/mvsdepth.hip)
def _f32(t, name, anchor=None):
    """a float32 contiguous device tensor (on the anchor's device) without its autograd history"""
    _need_cuda(t, name)
    if not t.is_floating_point():
        raise ValueError("pointnerf_amd: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    if anchor is not None and t.device != anchor.device:
        raise ValueError("pointnerf_amd: %s is on %s, expected %s" % (name, t.device, anchor.device))
    return t.detach().float().contiguous()


def mvs_cost_volume(features, proj, depth_values, align_corners=False):
    """pnerf_mvs_cost_volume: features [V,C,h,w] (one set shared by every batch item) or [B,V,C,h,w], proj [B,V,3,4] or [B,V,4,4] (the upper
    three rows are read, models/depth_estimators/module.py:47-48), depth_values [B,D] -> the variance volume [B,C,D,h,w] of
    mvsnet.py:110-122.  ``align_corners=False`` is what the reference's grid_sample call does under torch >= 1.3."""
    f = _f32(features, "features")
    if f.dim() == 4:
        f = f[None]
    if f.dim() != 5:
        raise ValueError("pointnerf_amd: features must be [V,C,h,w] or [B,V,C,h,w], got %s" % list(features.shape))
    dv = _f32(depth_values, "depth_values", f)
    if dv.dim() != 2:
        raise ValueError("pointnerf_amd: depth_values must be [B,D], got %s" % list(depth_values.shape))
    B, D = dv.shape
    sets, V, C, h, w = f.shape
    _need_cuda(proj, "proj")
    if proj.dim() != 4 or proj.shape[0] != B or proj.shape[1] != V or proj.shape[2] not in (3, 4) or proj.shape[3] != 4:
        raise ValueError("pointnerf_amd: proj must be [%d,%d,3 or 4,4], got %s" % (B, V, list(proj.shape)))
    p = _f32(proj[:, :, :3, :], "proj", f)
    lib = L.lib()
    nws = lib.pnerf_mvs_cost_volume_workspace_bytes(sets, V, h, w)
    ws = torch.empty(max(nws, 8), dtype=torch.uint8, device=f.device)
    vol = torch.empty(B, C, D, h, w, dtype=torch.float32, device=f.device)
    L.check(lib.pnerf_mvs_cost_volume(_ptr(f), sets, _ptr(p), _ptr(dv), B, V, C, D, h, w, 1 if align_corners else 0, _ptr(vol), _ptr(ws), nws,
                                      _stream()), "pnerf_mvs_cost_volume")
    return vol


def mvs_depth_regress(cost_reg, depth_values, return_prob=False):
    """pnerf_mvs_depth_regress: cost_reg [B,D,h,w] (logits), depth_values [B,D] -> (depth [B,h,w], photometric_confidence [B,h,w]) and, with
    ``return_prob``, the softmax [B,D,h,w] (mvsnet.py:127-136)."""
    c = _f32(cost_reg, "cost_reg")
    dv = _f32(depth_values, "depth_values", c)
    if c.dim() != 4 or dv.dim() != 2 or tuple(dv.shape) != tuple(c.shape[:2]):
        raise ValueError("pointnerf_amd: cost_reg [B,D,h,w] and depth_values [B,D] expected, got %s and %s" % (list(cost_reg.shape), list(depth_values.shape)))
    B, D, h, w = c.shape
    depth = torch.empty(B, h, w, dtype=torch.float32, device=c.device)
    conf = torch.empty(B, h, w, dtype=torch.float32, device=c.device)
    prob = torch.empty(B, D, h, w, dtype=torch.float32, device=c.device) if return_prob else None
    L.check(L.lib().pnerf_mvs_depth_regress(_ptr(c), _ptr(dv), B, D, h, w, _ptr(depth), _ptr(conf), _ptr(prob), _stream()), "pnerf_mvs_depth_regress")
    return (depth, conf, prob) if return_prob else (depth, conf)


def depth_to_cam_points(depth_lr, conf_lr, size, near_far, intrinsic):
    """pnerf_depth_to_cam_points: depth_lr / conf_lr [h,w] of one view, size = (H, W), near_far = (near, far), intrinsic [3,3] -> (cam_xyz
    [1,1,1,H,W,3], confidence [1,1,H,W], mask [1,1,H,W] bool): the tail of gen_points (models/mvs/mvs_points_model.py:329-337, 152-157,
    171-182, mvs_utils.py:92-98).  The inverse of the transposed intrinsics is taken by the host in float32, as the reference takes it."""
    d = _f32(depth_lr, "depth_lr")
    c = _f32(conf_lr, "conf_lr", d)
    if d.dim() != 2 or c.shape != d.shape:
        raise ValueError("pointnerf_amd: depth_lr and conf_lr must be [h,w], got %s and %s" % (list(depth_lr.shape), list(conf_lr.shape)))
    h, w = d.shape
    H, W = int(size[0]), int(size[1])
    K = torch.tensor(np.asarray(host_array(intrinsic) if isinstance(intrinsic, torch.Tensor) else intrinsic), dtype=torch.float32).reshape(3, 3)
    M = (ctypes.c_float * 9)(*torch.inverse(K.t()).contiguous().reshape(-1).tolist())
    nf = [float(v) for v in (host_array(near_far) if isinstance(near_far, torch.Tensor) else np.asarray(near_far)).reshape(-1)[:2]]
    xyz = torch.empty(1, 1, 1, H, W, 3, dtype=torch.float32, device=d.device)
    conf = torch.empty(1, 1, H, W, dtype=torch.float32, device=d.device)
    mask = torch.empty(1, 1, H, W, dtype=torch.uint8, device=d.device)
    L.check(L.lib().pnerf_depth_to_cam_points(_ptr(d), _ptr(c), h, w, H, W, nf[0], nf[1], M, _ptr(xyz), _ptr(conf), _ptr(mask), _stream()),
            "pnerf_depth_to_cam_points")
    return xyz, conf, mask.bool()


# ------------------------------------------------------------------------------------------ probe pass
PROBE_RAY_KEYS = (("ray_max_shading_opacity", 1), ("ray_max_sample_loc_w", 3), ("ray_max_far_dist", 1), ("shading_avg_color", 3),
                  ("shading_avg_dir", 3), ("shading_avg_conf", 1), ("shading_avg_embedding", 32))


def probe_rays(pts, opacity, weight, sample_loc, sample_pidx, ray_hit, R, SR, K):
    """pnerf_probe_rays: the ``opt.prob == 1`` outputs of the reference's ray marcher (neural_points_volumetric_model.py:331-352) for ALL R
    submitted rays from the renderer's dense tensors (opacity [R,SR], weight [R,SR,K], sample_loc [R,SR,3], sample_pidx [R,SR,K] i32, ray_hit [R]
    i32; ``pts`` = make_points(...) of the cloud), one launch, no host read.  Returns the seven tensors under the reference's key names, [R, C]
    each (C = 1, 3, 1, 3, 3, 1, 32 in the order of PROBE_RAY_KEYS); the rows of the rays that missed are zero."""
    R, SR, K = int(R), int(SR), int(K)
    f32, i32 = torch.float32, torch.int32
    _dense_args(None, None, ("opacity", opacity, f32, R * SR), ("weight", weight, f32, R * SR * K), ("sample_loc", sample_loc, f32, R * SR * 3),
                ("sample_pidx", sample_pidx, i32, R * SR * K), ("ray_hit", ray_hit, i32, R))
    out = {k: torch.empty(R, c, dtype=f32, device=opacity.device) for k, c in PROBE_RAY_KEYS}
    L.check(L.lib().pnerf_probe_rays(ctypes.byref(pts), _ptr(opacity), _ptr(weight), _ptr(sample_loc), _ptr(sample_pidx), _ptr(ray_hit), R, SR, K,
                                     *[_ptr(out[k]) for k, _ in PROBE_RAY_KEYS], _stream()), "pnerf_probe_rays")
    return out


def probe_hole_flags(ray_mask, max_opacity, far_dist, raycolor, gt, edge, bg, opacity_thresh, far_thresh=-1.0):
    """pnerf_probe_hole_mask: the candidate rule of probe_hole (run/train_ft.py:489-500) on the maps of one [H, W] view -> int32 0/1 flags
    [H, W] (``compact_valid`` turns them into the ascending candidate list).  ray_mask [H,W(,1)] int8, max_opacity / far_dist [H,W(,1)] f32,
    raycolor / gt [H,W,3] f32, edge [H,W] bool, bg: three numbers (read on the host)."""
    H, W = int(edge.shape[0]), int(edge.shape[1])
    n = H * W
    _need_cuda(edge, "edge")
    if edge.dtype != torch.bool or not edge.is_contiguous() or edge.dim() != 2:
        raise ValueError("pointnerf_amd: edge must be a contiguous [H, W] bool tensor")
    _dense_arg(ray_mask, "ray_mask", torch.int8, n); _dense_arg(max_opacity, "max_opacity", torch.float32, n); _dense_arg(far_dist, "far_dist", torch.float32, n)
    _dense_arg(raycolor, "raycolor", torch.float32, n * 3); _dense_arg(gt, "gt", torch.float32, n * 3)
    bg3 = (ctypes.c_float * 3)(*[float(x) for x in np.asarray(host_array(bg), dtype=np.float64).reshape(-1)[:3]])
    flags = torch.empty(H, W, dtype=torch.int32, device=edge.device)
    L.check(L.lib().pnerf_probe_hole_mask(_ptr(ray_mask), _ptr(max_opacity), _ptr(far_dist), _ptr(raycolor), _ptr(gt), _ptr(edge.view(torch.uint8)), bg3,
                                          H, W, float(opacity_thresh), float(far_thresh), _ptr(flags), _stream()), "pnerf_probe_hole_mask")
    return flags


# ------------------------------------------------------------------------------------------ depth and opacity maps
RAY_GEOMETRY_KEYS = ("acc", "depth_sum", "depth", "median_depth", "median_slot")


def ray_geometry(cam, sample_loc, sample_nn, ray_hit, opacity, blend_w):
    """pnerf_ray_geometry: per-ray accumulated opacity, expected camera-z depth and median depth of a render-only pass from the renderer's
    dense tensors (sample_loc [R,SR,3], sample_nn [R,SR] i32, ray_hit [R] i32, opacity / blend_w [R,SR] as render_forward returned them;
    ``cam`` = make_camera(...) of the view), one launch, no host read.  The depth is the one the reference's ``is_compute_depth`` was meant to
    give (neural_points_volumetric_model.py:318-322, with the camera-z depth for its undefined ``ray_ts``) on ray_march's blend weights
    (diff_ray_marching.py:508-554).  Returns dict(acc, depth_sum, depth = depth_sum / (acc + 1e-6), median_depth: [R] f32; median_slot: [R]
    i32, the lowest valid slot behind which the transmittance is below 0.5, -1 and depth 0 without one); rays that missed get zeros and -1.
    The four float tensors are the rows of ONE [4, R] allocation, handed out as well under "_rows" (in the order of RAY_GEOMETRY_KEYS), so that a
    caller that compacts them does it with one gather."""
    _need_cuda(sample_nn, "sample_nn")
    if sample_nn.dim() != 2:
        raise ValueError("pointnerf_amd: sample_nn must be [R, SR], got %s" % (list(sample_nn.shape),))
    R, SR = int(sample_nn.shape[0]), int(sample_nn.shape[1])
    f32, i32 = torch.float32, torch.int32
    _dense_args("sample_nn", sample_nn, ("sample_loc", sample_loc, f32, R * SR * 3), ("sample_nn", sample_nn, i32, R * SR), ("ray_hit", ray_hit, i32, R),
                ("opacity", opacity, f32, R * SR), ("blend_w", blend_w, f32, R * SR))
    dev = sample_nn.device
    rows = torch.empty(4, R, dtype=f32, device=dev)
    out = {k: rows[i] for i, k in enumerate(RAY_GEOMETRY_KEYS[:4])}
    out["median_slot"] = torch.empty(R, dtype=i32, device=dev)
    L.check(L.lib().pnerf_ray_geometry(ctypes.byref(cam), _ptr(sample_loc), _ptr(sample_nn), _ptr(ray_hit), _ptr(opacity), _ptr(blend_w), R, SR,
                                       *[_ptr(out[k]) for k in RAY_GEOMETRY_KEYS], _stream()), "pnerf_ray_geometry")
    out["_rows"] = rows
    return out


def geometry_canvas(pixel_idx, ray_mask, depth, median_depth, acc, canvases, flag=None):
    """pnerf_geometry_canvas: the values of one chunk of rays written into the three [H, W] float32 canvases ``canvases`` = (depth, median_depth,
    acc) at the rays' pixels: pixel_idx [n, 2] (px, py; converted to int32 when it is not), ray_mask [n] int8 or None (a ray with mask <= 0
    writes 0), depth / median_depth / acc [n] f32.  One launch in the place of three index-puts; no other pixel is touched.
    A pixel outside the image is an error the DEVICE finds: with ``flag`` = None the call reads its flag back and raises; a caller that fills an
    image in several chunks passes ``flag`` = canvas_flag(device) to every call (nothing is read in between) and calls check_canvas_flag(flag)
    once, when it reads the canvases."""
    _need_cuda(pixel_idx, "pixel_idx")
    n = int(pixel_idx.numel()) // 2
    if pixel_idx.dtype != torch.int32 or not pixel_idx.is_contiguous():
        pixel_idx = pixel_idx.to(torch.int32).contiguous()
    _dense_arg(pixel_idx, "pixel_idx", torch.int32, n * 2)
    if ray_mask is not None:
        _dense_arg(ray_mask, "ray_mask", torch.int8, n)
    f32 = torch.float32
    _dense_arg(depth, "depth", f32, n); _dense_arg(median_depth, "median_depth", f32, n); _dense_arg(acc, "acc", f32, n)
    if len(canvases) != 3 or canvases[0].dim() != 2:
        raise ValueError("pointnerf_amd: canvases must be three [H, W] tensors (depth, median_depth, acc)")
    H, W = int(canvases[0].shape[0]), int(canvases[0].shape[1])
    for name, t in zip(("depth canvas", "median_depth canvas", "acc canvas"), canvases):
        _dense_arg(t, name, f32, H * W)
    own = flag is None
    if own:
        flag = canvas_flag(pixel_idx.device)
    _dense_arg(flag, "flag", torch.int32, 1)
    L.check(L.lib().pnerf_geometry_canvas(_ptr(pixel_idx), _ptr(ray_mask), _ptr(depth), _ptr(median_depth), _ptr(acc), n, H, W,
                                          _ptr(canvases[0]), _ptr(canvases[1]), _ptr(canvases[2]), _ptr(flag), _stream()), "pnerf_geometry_canvas")
    if own:
        check_canvas_flag(flag)
    return flag


def canvas_flag(device):
    """the zeroed device word geometry_canvas reports a pixel outside the image in"""
    return torch.zeros(1, dtype=torch.int32, device=device)


def check_canvas_flag(flag):
    """reads a geometry_canvas flag back (one host read) and raises what the library stored there"""
    L.check(int(flag.cpu()[0]), "pnerf_geometry_canvas (a pixel_idx outside the canvas)")


# ------------------------------------------------------------------------------------------ point attribute maps, picking, lifting
RAY_ATTRIBUTES_CMAX, LIFT_CMAX = 256, 8


def _ray_entries(blend_w, weight, sample_pidx, ray_hit):
    """the four dense tensors both point-map ops read, checked by name -> (R, SR, K)"""
    _need_cuda(weight, "weight")
    if weight.dim() != 3:
        raise ValueError("pointnerf_amd: weight must be [R, SR, K], got %s" % (list(weight.shape),))
    R, SR, K = (int(x) for x in weight.shape)
    f32, i32 = torch.float32, torch.int32
    _dense_args("weight", weight, ("blend_w", blend_w, f32, R * SR), ("weight", weight, f32, R * SR * K), ("sample_pidx", sample_pidx, i32, R * SR * K),
                ("ray_hit", ray_hit, i32, R))
    return R, SR, K


def ray_attributes(attr, blend_w, weight, sample_pidx, ray_hit, n_points=None):
    """pnerf_ray_attributes: a per-point table seen through the render, and the point behind every ray, from the renderer's dense tensors
    (blend_w [R,SR], weight [R,SR,K], sample_pidx [R,SR,K] i32, ray_hit [R] i32 as render_dense leaves them), one launch, no host read.
    With g[r,s,k] = blend_w[r,s] * weight[r,s,k] (0 where sample_pidx is outside [0, n_points): the empty slot -1 reads no point; the
    confidence factor of the density is not part of g) and ``attr`` [n_points, C] float32, C <= 256:
      attr_sum [R, C] = sum_{s,k} g attr[sample_pidx]  (fp32, fixed order, no atomics: two calls give the same bits);
      top_flat [R] i32 = the lowest flat index s*K + k among the maxima of g[r] -- the largest single (sample, slot) entry, not a per-point
      sum over the ray's samples --, top_point [R] i32 = sample_pidx there, top_contrib [R] = g there; -1 / -1 / 0 where no g is > 0.
    Rays that missed get zeros and -1.  ``n_points`` (default: the rows of ``attr``) may be smaller than the table.  ``attr`` = None runs the
    pick only (attr_sum is [R, 0]); without ``n_points`` every index >= 0 then counts."""
    R, SR, K = _ray_entries(blend_w, weight, sample_pidx, ray_hit)
    f32, i32, dev = torch.float32, torch.int32, weight.device
    C = 0
    if attr is not None:
        _need_cuda(attr, "attr")
        if attr.dim() != 2:
            raise ValueError("pointnerf_amd: attr must be [n_points, C], got %s" % (list(attr.shape),))
        _dense_arg(attr, "attr", f32)
        n_points, C = int(attr.shape[0]) if n_points is None else int(n_points), int(attr.shape[1])
        if n_points > int(attr.shape[0]):
            raise ValueError("pointnerf_amd: n_points %d exceeds the %d rows of attr" % (n_points, int(attr.shape[0])))
        if C > RAY_ATTRIBUTES_CMAX:
            raise ValueError("pointnerf_amd: attr has %d columns, pnerf_ray_attributes takes at most %d" % (C, RAY_ATTRIBUTES_CMAX))
    elif n_points is None:
        n_points = 2 ** 31 - 1                                            # no table to stay inside: every index >= 0 counts
    out = dict(attr_sum=torch.empty(R, C, dtype=f32, device=dev), top_point=torch.empty(R, dtype=i32, device=dev),
               top_flat=torch.empty(R, dtype=i32, device=dev), top_contrib=torch.empty(R, dtype=f32, device=dev))
    L.check(L.lib().pnerf_ray_attributes(_ptr(attr if C else None), int(n_points), C, _ptr(blend_w), _ptr(weight), _ptr(sample_pidx), _ptr(ray_hit),
                                         R, SR, K, _ptr(out["attr_sum"] if C else None), _ptr(out["top_point"]), _ptr(out["top_flat"]),
                                         _ptr(out["top_contrib"]), _stream()), "pnerf_ray_attributes")
    return out


def lift_to_points(values, ray_factor, blend_w, weight, sample_pidx, ray_hit, n_points, out=None):
    """pnerf_lift_to_points, the adjoint of ray_attributes: per-ray ``values`` [R, C] float32 (C <= 8; None: C = 0) times the optional per-ray
    factor ``ray_factor`` [R] float32 (None: 1) spread onto the points with the same g: point_sum[p, c] += g m[r] values[r, c],
    point_mass[p] += g m[r] over every entry that addresses p.  Returns (point_sum [n_points, C], point_mass [n_points]); ``out`` = None
    allocates zeroed accumulators, ``out`` = (point_sum, point_mass) ADDS into the caller's, so that several views add up.  The sums are
    fp32 atomicAdd on global memory (like the backward's point gradients): they depend on arrival order and are NOT bit-reproducible."""
    R, SR, K = _ray_entries(blend_w, weight, sample_pidx, ray_hit)
    f32, dev, n_points = torch.float32, weight.device, int(n_points)
    C = 0
    if values is not None:
        _need_cuda(values, "values")
        if values.dim() != 2:
            raise ValueError("pointnerf_amd: values must be [R, C], got %s" % (list(values.shape),))
        C = int(values.shape[1])
        if C > LIFT_CMAX:
            raise ValueError("pointnerf_amd: values has %d columns, pnerf_lift_to_points takes at most %d" % (C, LIFT_CMAX))
        _dense_arg(values, "values", f32, R * C)
    if ray_factor is not None:
        _dense_arg(ray_factor, "ray_factor", f32, R)
    if out is None:
        out = (torch.zeros(n_points, C, dtype=f32, device=dev), torch.zeros(n_points, dtype=f32, device=dev))
    point_sum, point_mass = out
    _need_cuda(point_sum, "out[0]")
    if point_sum.dim() != 2 or int(point_sum.shape[1]) != C:
        raise ValueError("pointnerf_amd: out[0] must be [n_points, %d], got %s" % (C, list(point_sum.shape)))
    _dense_arg(point_sum, "out[0]", f32, n_points * C); _dense_arg(point_mass, "out[1]", f32, n_points)
    L.check(L.lib().pnerf_lift_to_points(_ptr(values if C else None), C, _ptr(ray_factor), _ptr(blend_w), _ptr(weight), _ptr(sample_pidx), _ptr(ray_hit),
                                         R, SR, K, n_points, _ptr(point_sum if C else None), _ptr(point_mass), _stream()), "pnerf_lift_to_points")
    return point_sum, point_mass


# ------------------------------------------------------------------------------------------ profiling
def mfma_rate_tflops(mode=2, ms_target=60.0, device=None):
    """TFLOP/s of register-resident v_mfma_f32_32x32x16_f16 on the whole chip (pnerf_debug_mfma_rate; mode 0 zero operands, 1 one constant,
    2 pseudo-random f16: operands that toggle like a GEMM's): the matrix-pipe ceiling bench.py reports beside the nominal 2.5 PFLOP/s.
    The clock needs time to come up from idle and to settle under the power management: launches of ~``ms_target`` are repeated until two
    consecutive ones agree to 3 % (at most eight) and the last one is reported -- the SUSTAINED rate (the first launches of a cold process run at the
    clock's way up from idle, the first ones with toggling operands at a clock the power management has not yet taken back)."""
    import ctypes
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    scratch = torch.zeros(256, dtype=torch.float32, device=dev)
    flop = ctypes.c_double(0.0)
    iters = max(int(ms_target / 1000.0 * 2.4e9 / (2 * 32 * 32)), 64)          # two waves per SIMD x 32 MFMAs of 32 cycles per iteration
    last = 0.0
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(L.lib().pnerf_debug_mfma_rate(int(mode), int(iters), _ptr(scratch), ctypes.byref(flop), _stream()), "pnerf_debug_mfma_rate")
        e1.record()
        e1.synchronize()
        rate = flop.value / (e0.elapsed_time(e1) * 1e-3) / 1e12
        settled = last > 0.0 and abs(rate - last) <= 0.03 * last
        last = rate
        if settled:
            break
    return last


def prof_enable(on=True):
    L.lib().pnerf_prof_enable(1 if on else 0)


def prof_collect():
    """{kernel name: (total ms, launches)} since the last collect; synchronises the device."""
    lib = L.lib()
    n = lib.pnerf_prof_kernel_count()
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    L.check(lib.pnerf_prof_collect(ms, cnt), "pnerf_prof_collect")
    return {lib.pnerf_prof_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}

"""pnerf_probe_rays / pnerf_probe_hole_mask (pointnerf_amd/csrc/probe.hip: the probe pass of the point-growing step) on the host emulator
(tools/emu): the real kernel code, every GPU thread a fiber, through ops.probe_rays / ops.probe_hole_flags, against the torch restatement
and the bars of tests/probe_case.py and against BOTH statements of the candidate rule (probe.hole_mask in ATen, pyref.probe_hole_mask as
index loops).  Selection, tie, chunking, empty-slot and border errors show without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import probe_case as C
from emu_util import emu_backend
from pointnerf_amd import ops


@pytest.fixture(autouse=True)
def _emu():
    with emu_backend():
        yield


def _make_points(pts):
    return ops.make_points(pts["xyz"], pts["points_embeding"], pts["points_conf"], pts["points_dir"], pts["points_color"])


@pytest.mark.parametrize("near0", [True, False])
@pytest.mark.parametrize("R,SR,K", C.RAY_CASES)
def test_emulated_probe_rays_match_the_restatement(R, SR, K, near0):
    pts, c = C.points(near0), C.ray_case(R, SR, K)
    C.assert_case_covers(pts, c, near0)
    ref, scale = C.restate(pts, c)
    got = ops.probe_rays(_make_points(pts), c["opacity"], c["weight"], c["sample_loc"], c["sample_pidx"], c["ray_hit"], R, SR, K)
    assert tuple(got) == C.KEYS and all(got[k].shape == (R, w) for k, w in ops.PROBE_RAY_KEYS)
    C.check(got, ref, scale, "R%d SR%d K%d near0=%d" % (R, SR, K, near0))
    for r in range(3, R, 4):                                  # the rays that missed: exact zeros although their input rows are NaN
        assert all(float(got[k][r].abs().max()) == 0.0 for k in C.KEYS)


def test_emulated_probe_rays_argument_errors():
    from pointnerf_amd import _lib as L
    lib = L.lib()
    pts, c = C.points(True), C.ray_case(5, 24, 8)
    P = _make_points(pts)
    out = {k: torch.zeros(5, w) for k, w in ops.PROBE_RAY_KEYS}
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ins = [c[k] for k in ("opacity", "weight", "sample_loc", "sample_pidx", "ray_hit")]

    def call(R, SR, K, pts_=P, drop=None):
        args = [p(t) for t in ins] + [R, SR, K] + [p(out[k]) for k, _ in ops.PROBE_RAY_KEYS]
        if drop is not None:
            args[drop] = None
        return lib.pnerf_probe_rays(ctypes.byref(pts_), *args, None)

    assert call(5, 24, 8) == 0
    assert call(5, 24, 0) == -1 and call(5, 24, 17) == -1 and call(5, 0, 8) == -1 and call(-1, 24, 8) == -1          # PNERF_E_INVAL
    assert call(5, 24, 8, drop=0) == -1 and call(5, 24, 8, drop=4) == -1 and call(5, 24, 8, drop=14) == -1             # a null pointer
    before = {k: v.clone() for k, v in out.items()}
    assert call(0, 24, 8) == 0 and all(torch.equal(out[k], before[k]) for k in out)                                      # R == 0: nothing runs
    narrow = ops.make_points(pts["xyz"], pts["points_embeding"][:, :16].contiguous(), pts["points_conf"], pts["points_dir"], pts["points_color"])
    assert call(5, 24, 8, pts_=narrow) == -4                                                                             # PNERF_E_UNSUP: not 32 wide
    with pytest.raises(ValueError):                            # a weight table of another K would be read out of bounds
        ops.probe_rays(P, c["opacity"], c["weight"][..., :4].contiguous(), c["sample_loc"], c["sample_pidx"], c["ray_hit"], 5, 24, 8)
    with pytest.raises(ValueError):
        ops.probe_rays(P, c["opacity"], c["weight"], c["sample_loc"], c["sample_pidx"].long(), c["ray_hit"], 5, 24, 8)


@pytest.mark.parametrize("far_thresh", [-1.0, C.FAR_THRESH])
@pytest.mark.parametrize("H,W", C.MASK_CASES)
def test_emulated_hole_mask_equals_both_statements_of_the_rule(H, W, far_thresh):
    c = C.mask_case(H, W)
    aten, loops = C.mask_references(c, far_thresh)
    flags = ops.probe_hole_flags(c["ray_mask"], c["ray_max_shading_opacity"], c["ray_max_far_dist"], c["coarse_raycolor"], c["gt"], c["edge"],
                                 c["bg"], C.OPACITY_THRESH, far_thresh)
    assert flags.dtype == torch.int32 and flags.shape == (H, W) and set(np.unique(flags.numpy()).tolist()) <= {0, 1}
    got = flags.numpy() > 0
    assert np.array_equal(got, aten) and np.array_equal(got, loops), (got.astype(int), aten.astype(int), loops.astype(int))
    if H * W > 1:
        assert 0 < got.sum() < H * W
    # the candidate list: the flags through the existing compaction, ascending row-major, count on the device
    cand, counters = ops.compact_valid(flags.reshape(-1))
    n = int(counters[0])
    assert n == int(got.sum()) and np.array_equal(cand[:n].numpy(), np.nonzero(got.reshape(-1))[0])


def test_emulated_hole_mask_argument_errors():
    c = C.mask_case(5, 7)
    args = (c["ray_mask"], c["ray_max_shading_opacity"], c["ray_max_far_dist"], c["coarse_raycolor"], c["gt"], c["edge"], c["bg"], 0.4)
    with pytest.raises(ValueError):
        ops.probe_hole_flags(c["ray_mask"].float(), *args[1:])
    with pytest.raises(ValueError):
        ops.probe_hole_flags(*args[:5], c["edge"].to(torch.uint8), c["bg"], 0.4)
    from pointnerf_amd import _lib as L
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    bg3 = (ctypes.c_float * 3)(1.0, 1.0, 1.0)
    flags = torch.zeros(5, 7, dtype=torch.int32)
    ptrs = [p(t) for t in args[:5]] + [p(c["edge"].view(torch.uint8))]
    lib = L.lib()
    assert lib.pnerf_probe_hole_mask(*ptrs, bg3, 5, 7, 0.4, -1.0, p(flags), None) == 0
    assert lib.pnerf_probe_hole_mask(*ptrs, bg3, 0, 7, 0.4, -1.0, p(flags), None) == -1 and lib.pnerf_probe_hole_mask(*ptrs, bg3, 5, -1, 0.4, -1.0, p(flags), None) == -1
    assert lib.pnerf_probe_hole_mask(*ptrs, None, 5, 7, 0.4, -1.0, p(flags), None) == -1 and lib.pnerf_probe_hole_mask(*ptrs, bg3, 5, 7, 0.4, -1.0, None, None) == -1

"""The four render entry points (pnerf_render_forward / _backward, pnerf_agg_forward / _backward) validate their arguments in ONE routine
(csrc/render.hip: check_step) before any HIP call, so it runs here, on the real library, without a GPU.  Every case below is a well-formed
call with ONE defect (two where the order of the checks decides between two codes): the addresses are dummies that are never dereferenced,
and no call of this file gets past the validation.  The expected codes were written down from the source of the commit before the step
record (its check_common + the per-entry null lists, in its order), not from running this one; the three marked NEW have no counterpart
there (the entry point had no such parameter)."""
import ctypes

import pytest

from pointnerf_amd import _lib as L

OK, INVAL, WS, UNSUP = 0, -1, -2, -4
R, SR, K, CAP = 4, 2, 3, 8
ADDR = 0x10000                      # non-null, 16-byte aligned, never dereferenced
ENTRIES = ("pnerf_render_forward", "pnerf_render_backward", "pnerf_agg_forward", "pnerf_agg_backward")
STEP_PTRS = ("raydir", "sample_loc", "sample_pidx", "valid_list", "counters", "params", "packed_mlp")
# the pointers of the call itself, after (cam, pts, step) and before (ws, ws_bytes, stream)
CALL_PTRS = {"pnerf_render_forward": ("decoded", "weight", "ray_color", "opacity", "bg_trans", "blend_w", "saved"),
             "pnerf_render_backward": ("decoded", "weight", "grad_ray_color", "saved", "grad_params", "pg"),
             "pnerf_agg_forward": ("decoded", "weight", "saved"),
             "pnerf_agg_backward": ("decoded", "weight", "grad_decoded", "saved", "grad_params", "pg")}


def _forward(entry):
    return entry.endswith("_forward")


def _render(entry):
    return entry.startswith("pnerf_render")


def _ws_needed(entry):
    lib = L.lib()
    if _forward(entry):
        return lib.pnerf_agg_workspace_bytes(CAP, K)
    return lib.pnerf_render_backward_workspace_bytes(R, SR) if _render(entry) else lib.pnerf_render_backward_workspace_bytes(0, 1)


def _call(entry, step={}, pts={}, call={}, cam=True, with_pts=True, with_step=True, ws=ADDR, ws_bytes=None):
    """the well-formed call of ``entry`` with the given fields replaced"""
    c, p, s, pg = L.Camera(), L.Points(), L.Step(), L.PointGrads()
    p.xyz = p.embedding = p.conf = p.dir = p.color = ADDR
    p.n, p.feat_dim = 10, 32
    for k, v in pts.items():
        setattr(p, k, v)
    for k in STEP_PTRS + (("sample_nn",) if _render(entry) else ()):
        setattr(s, k, ADDR)
    s.R, s.SR, s.K, s.n_valid_max = R, SR, K, CAP
    for k, v in step.items():
        setattr(s, k, v)
    pg.embedding = pg.conf = pg.dir = pg.color = ADDR
    args = dict.fromkeys(CALL_PTRS[entry], ADDR)
    if _forward(entry):
        args["saved"] = None                       # an inference forward
    else:
        args["pg"] = ctypes.byref(pg)
    args.update(call)
    return getattr(L.lib(), entry)(ctypes.byref(c) if cam else None, ctypes.byref(p) if with_pts else None, ctypes.byref(s) if with_step else None,
                                   *[args[k] for k in CALL_PTRS[entry]], ws, _ws_needed(entry) if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_pointer_is_invalid(entry):
    assert _call(entry, cam=False) == INVAL and _call(entry, with_pts=False) == INVAL and _call(entry, with_step=False) == INVAL
    for k in STEP_PTRS + (("sample_nn",) if _render(entry) else ()):
        assert _call(entry, step={k: None}) == INVAL, k
    for k in CALL_PTRS[entry]:
        if not (_forward(entry) and k == "saved"):             # (a forward without a saved area is an inference forward)
            assert _call(entry, call={k: None}) == INVAL, k
    if not _forward(entry):
        assert _call(entry, ws=None) == INVAL
    # a point array: "configuration not supported" (check_common's third line), not "bad argument"
    for k in ("xyz", "embedding", "conf", "dir", "color"):
        assert _call(entry, pts={k: None}) == UNSUP, k


@pytest.mark.parametrize("entry", ENTRIES)
def test_perspective_coordinates_come_together(entry):
    # pnerf_agg_forward: the parent's own check; NEW for the other three (pnerf_agg_backward takes its forward's record, the render pair none)
    assert _call(entry, step={"xyz_pers": ADDR}) == INVAL and _call(entry, step={"loc_pers": ADDR}) == INVAL
    if _render(entry):
        assert _call(entry, step={"xyz_pers": ADDR, "loc_pers": ADDR}) == INVAL          # NEW: the render pair projects from the camera


@pytest.mark.parametrize("entry", ENTRIES)
def test_sizes_out_of_range(entry):
    for bad in ({"K": 0}, {"K": 17}, {"K": -1}, {"SR": 0}, {"R": -1}):
        assert _call(entry, step=bad) == INVAL, bad
    assert _call(entry, pts={"feat_dim": 16}) == UNSUP
    # the order of the parent's check_common: sizes, then the feature width, then everything else
    assert _call(entry, step={"K": 17}, pts={"feat_dim": 16}) == INVAL
    assert _call(entry, step={"raydir": None}, pts={"feat_dim": 16}) == UNSUP
    assert _call(entry, step={"R": 0}, pts={"feat_dim": 16}) == UNSUP


@pytest.mark.parametrize("entry", ENTRIES)
def test_per_point_frames_are_render_only(entry):
    if _forward(entry):
        assert _call(entry, pts={"frames": ADDR}, call={"saved": ADDR}) == INVAL         # a training forward
        assert _call(entry, pts={"frames": ADDR}, call={"saved": ADDR}, step={"R": 0}) == INVAL      # before the R == 0 return
    else:
        assert _call(entry, pts={"frames": ADDR}) == INVAL
        assert _call(entry, pts={"frames": ADDR}, ws_bytes=0) == INVAL                   # before the workspace check


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_too_small_and_empty_calls(entry):
    need = _ws_needed(entry)
    assert need > 0
    assert _call(entry, ws_bytes=need - 1) == WS
    assert _call(entry, step={"R": 0}) == OK
    if _forward(entry):
        assert _call(entry, ws=None) == WS                                               # a missing inference workspace is a too-small one
        assert _call(entry, step={"R": 0}, ws_bytes=0) == OK                             # the R == 0 return precedes the workspace check
    else:
        assert _call(entry, step={"n_valid_max": 0}) == OK
        empty = L.lib().pnerf_render_backward_workspace_bytes(0, 1)                      # R == 0: no [R,SR,4] gradient, the partials only
        assert _call(entry, step={"R": 0}, ws_bytes=empty - 1) == WS                     # the workspace check precedes both empty returns
        assert _call(entry, step={"n_valid_max": 0}, ws_bytes=need - 1) == WS

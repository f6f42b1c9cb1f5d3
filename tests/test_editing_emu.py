"""Per-point Rw2c frames on the host emulator (tools/emu: the FRAMES instances of k_agg_forward / k_color_forward compiled for the host):
the fused NeuralPointsRayMarching forward and the level-1 chain on small_k4 with 3-part frames against the restatement of the reference's
per-point branch (tests/editing_case.py).  Without the feature the fused path renders every point with point 0's frame (0.2 off in
``decoded``) and the level-1 chain raises."""
import pytest
import torch

import editing_case as E
import test_gpu_level1 as T1
from emu_util import emu_backend


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(T1, "DEV", "cpu")
    with emu_backend():
        yield


def test_emulated_fused_forward_with_frames_matches_the_restatement():
    E.check_fused("small_k4", "cpu")


def test_emulated_level1_chain_with_frames_matches_the_restatement():
    E.check_level1("small_k4", "cpu")


def test_emulated_training_with_frames_raises():
    E.check_training_raises("small_k4", "cpu")


def test_emulated_library_refuses_frames_outside_the_render_path():
    """C ABI: frames with a training forward / in a backward -> PNERF_E_INVAL; with an arithmetic no FRAMES instance serves -> the Python
    layer names the setting (the library itself answers PNERF_E_UNSUP)"""
    import ctypes
    from gpu_util import hip_render
    from pointnerf_amd import ops
    (opt, xyz, attrs, inp, mlp), frames, _ = E.reference("small_k4")
    dense, fwd, ctx = hip_render(opt, xyz, attrs, inp, mlp, train=False)
    ft = ops.frames_table(frames, xyz.shape[0])
    pts = ops.make_points(ctx["xyz"], *[ctx["pts_t"][k] for k in ("points_embeding", "points_conf", "points_dir", "points_color")], frames=ft)
    assert pts.frames == ft.data_ptr()
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
        ops.render_forward(ctx["cam"], pts, ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], True)
    grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
    with pytest.raises(RuntimeError, match="PNERF_E_INVAL"):
        f2 = dict(fwd, saved=torch.zeros(1 << 16, dtype=torch.uint8))
        ops.render_backward(ctx["cam"], pts, ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], f2,
                            torch.zeros(ctx["R"], 3), torch.zeros_like(ctx["flat"]), grads)
    old = ops.set_inference_products(2)
    try:
        with pytest.raises(NotImplementedError, match="set_inference_products"):
            ops.frames_table(frames, xyz.shape[0])
        with pytest.raises(RuntimeError, match="PNERF_E_UNSUP"):
            ops.render_forward(ctx["cam"], pts, ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], False)
    finally:
        ops.set_inference_products(old)
    oldc = ops.set_cross_terms(8, where=5)
    try:
        with pytest.raises(NotImplementedError, match="cross"):
            ops.frames_table(frames, xyz.shape[0])
        with pytest.raises(RuntimeError, match="PNERF_E_UNSUP"):
            ops.render_forward(ctx["cam"], pts, ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], False)
    finally:
        ops.set_cross_terms(oldc[0], where=oldc[1])
    ops.frames_table(frames, xyz.shape[0])            # (settings restored)


def test_emulated_level1_refuses_a_mask_with_an_empty_slot_0():
    """a caller-made neighbor mask may leave slot 0 of a valid sample empty (the query never does): with per-point frames the view direction's
    frame would come from another sample's pseudo point -- refused, not rendered wrong"""
    (opt, xyz, attrs, inp, mlp), frames, ref = E.reference("small_k4")
    model, d = E.build_model("small_k4", "cpu", frames)
    npnt, agg = model.neural_points, model.aggregator
    with torch.no_grad():
        tup = list(npnt({"pixel_idx": d["pixel_idx"], "camrotc2w": d["camrotc2w"], "campos": d["campos"], "near": d["near"], "far": d["far"],
                         "focal": None, "h": d["h"], "w": d["w"], "intrinsic": d["intrinsic"], "gt_image": d["gt_image"], "raydir": d["raydir"]}))
        assert tup[1].shape == tup[7].shape + (3, 3)                                     # the gathered frames [1,R'',SR,K,3,3]
        mask = tup[7].clone()
        two = (mask.sum(-1) >= 2).nonzero()[0]
        mask[two[0], two[1], two[2], 0] = False
        args = tup[:7] + [mask] + tup[8:11] + tup[12:14]
        with pytest.raises(NotImplementedError, match="slot 0"):
            agg(*args)

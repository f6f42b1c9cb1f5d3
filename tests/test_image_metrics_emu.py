"""pnerf_image_metrics (pointnerf_amd/csrc/metrics.hip: the SSIM / MSE scorer of the evaluation) on the host emulator (tools/emu):
the real kernel code, every GPU thread a fiber, against the float64 numpy / scipy restatement of skimage's steps in
tests/image_metrics_case.py (skimage is not installed here).  Index, halo, normalisation and synchronisation errors show without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import image_metrics_case as C
from emu_util import emu_backend
from pointnerf_amd import eval_loop, ops


@pytest.fixture(autouse=True)
def _emu():
    with emu_backend():
        yield


# 11 x 11: a single window; 12 x 19: one partial tile; 27 x 28: 17 x 18 windows, one past the tile edge (16) in both directions
@pytest.mark.parametrize("data_range", [2.0, 1.0])
@pytest.mark.parametrize("quantize8", [False, True])
@pytest.mark.parametrize("H,W", [(11, 11), (12, 19), (27, 28)])
def test_emulated_scores_match_the_float64_yardstick(H, W, quantize8, data_range):
    img, gt = C.tensors(H, W)
    got = ops.image_metrics(img, gt, data_range=data_range, quantize8=quantize8)
    assert got.dtype == torch.float64 and got.shape == (2,)
    C.check(float(got[0]), float(got[1]), C.reference(H, W, data_range, quantize8), "%dx%d q%d R%g" % (H, W, quantize8, data_range))


def test_emulated_identical_images_score_exactly_one():
    img = C.tensors(27, 28)[0]
    for q in (False, True):
        got = ops.image_metrics(img, img.clone(), quantize8=q)
        assert float(got[0]) == 0.0 and float(got[1]) == 1.0
    assert float(eval_loop.image_scores(img, img.clone())["psnr"]) == float("inf")


def test_emulated_argument_errors():
    from pointnerf_amd import _lib as L
    lib = L.lib()
    img = torch.zeros(12, 19, 3)
    out = torch.zeros(4, dtype=torch.float64)
    need = lib.pnerf_image_metrics_workspace_bytes(12, 19, 11)
    ws = torch.zeros(need, dtype=torch.uint8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda H, W, win, R, nbytes: lib.pnerf_image_metrics(p(img), p(img), H, W, win, R, 1, p(out), p(ws), nbytes, None)
    assert need >= 32 and call(12, 19, 11, 2.0, need) == 0
    assert call(10, 19, 11, 2.0, need) == -1 and call(12, 10, 11, 2.0, need) == -1          # H < win, W < win: PNERF_E_INVAL
    assert call(12, 19, 10, 2.0, need) == -1 and call(12, 19, 1, 2.0, need) == -1            # even win, win < 3
    assert call(12, 19, 11, 0.0, need) == -1                                                 # data_range <= 0
    assert lib.pnerf_image_metrics(None, p(img), 12, 19, 11, 2.0, 1, p(out), p(ws), need, None) == -1
    assert call(12, 19, 11, 2.0, need - 1) == -2                                             # PNERF_E_WS
    big = torch.zeros(27, 27, 3)                                                             # win = 27 > 25: the tile no longer fits the LDS
    assert lib.pnerf_image_metrics(p(big), p(big), 27, 27, 27, 2.0, 1, p(out), p(ws), need, None) == -4         # PNERF_E_UNSUP
    assert lib.pnerf_image_metrics(p(big), p(big), 27, 27, 25, 2.0, 0, p(out), p(ws), need, None) == 0 and float(out[1]) == 9.0
    with pytest.raises(TypeError):
        ops.image_metrics(img.double(), img.double())
    with pytest.raises(ValueError):
        ops.image_metrics(torch.zeros(12, 19, 4), torch.zeros(12, 19, 4))
    with pytest.raises(ValueError):
        ops.image_metrics(torch.zeros(12, 3, 19).permute(0, 2, 1), img)


def test_emulated_image_scores_names_and_formulas():
    img, gt = C.tensors(12, 19)
    both = ops.image_metrics(img, gt)
    s = eval_loop.image_scores(img, gt)
    assert sorted(s) == ["psnr", "rmse", "ssim"] and all(v.dim() == 0 and v.dtype == torch.float64 for v in s.values())
    mse = float(both[0])
    assert abs(float(s["psnr"]) - 10.0 * np.log10(1.0 / mse)) <= 1e-12 and abs(float(s["rmse"]) - np.sqrt(mse)) <= 1e-15
    assert float(s["ssim"]) == float(both[1])
    assert list(eval_loop.image_scores(img, gt, metrics=("rmse",))) == ["rmse"]
    for name in ("lpips", "vgglpips"):
        with pytest.raises(NotImplementedError, match="weights"):
            eval_loop.image_scores(img, gt, metrics=("psnr", name))
    with pytest.raises(NotImplementedError, match="metrics of fid not implemented"):
        eval_loop.image_scores(img, gt, metrics=("fid",))
    with pytest.raises(NotImplementedError, match="weights"):          # test_views refuses the name before it touches model or views
        eval_loop.test_views(None, [], None, 24, 32, metrics=("ssim", "lpips"))

"""Shared by tests/test_image_metrics_emu.py and tests/test_gpu_image_metrics.py: the seeded image pairs and the float64 yardstick of
pnerf_image_metrics.

The yardstick restates, step by step in numpy / scipy float64, what the reference's evaluation computes (run/evaluate.py:55-61,76 on the
PNGs of utils/visualizer.py:58-59): skimage's ``structural_similarity(gt, img, win_size=11, multichannel=True)`` (uniform_filter with
reflected borders on the five moment planes, the covariance scaled by NP / (NP - 1), the formula, the crop of (win - 1) / 2 pixels, the
mean per channel and the mean over the channels) and ``mean_squared_error``.  skimage itself is not installed where these tests run
(and only versions <= 0.18 accept the reference's call), which is why its steps are written out here; scipy.ndimage is.
"""
import numpy as np
from scipy.ndimage import uniform_filter

T = 16          # tile edge of k_image_metrics (PN_IM_T in pointnerf_amd/csrc/metrics.hip), in window positions
WIN = 11

SSIM_BAR = 1e-9


def mse_bar(mse):
    return 1e-12 + 1e-9 * mse


def quantize(x):
    """utils/visualizer.py:58-59 (uint8 conversion: truncation) followed by run/evaluate.py:55 (float32 / 255)"""
    x = np.asarray(x, np.float32)
    return (np.clip(x, 0, 1) * 255).astype(np.uint8).astype(np.float32) / np.float32(255.0)


def yardstick(img, gt, win=WIN, data_range=2.0, quantize8=True):
    """dict(mse, ssim, ssim_channels [3]) in float64"""
    img, gt = np.asarray(img, np.float32), np.asarray(gt, np.float32)
    if quantize8:
        img, gt = quantize(img), quantize(gt)
    x, y = gt.astype(np.float64), img.astype(np.float64)
    H, W, _ = x.shape
    NP = win * win
    cov = NP / (NP - 1.0)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    pad = (win - 1) // 2
    per_channel = []
    for c in range(3):
        a, b = x[..., c], y[..., c]
        ux, uy = uniform_filter(a, size=win), uniform_filter(b, size=win)
        uxx, uyy, uxy = uniform_filter(a * a, size=win), uniform_filter(b * b, size=win), uniform_filter(a * b, size=win)
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        per_channel.append(S[pad:H - pad, pad:W - pad].mean())
    return dict(mse=float(np.mean((x - y) ** 2)), ssim=float(np.mean(per_channel)), ssim_channels=np.asarray(per_channel))


_pairs = {}


def pair(H, W):
    """(img, gt) float32 [H, W, 3], seeded: gt a smooth sinusoid pattern per channel in [0, 1] with the top third of the rows exactly 1.0
    (the white background), img = gt + 0.05 * normal noise with the same flat third.  Computed once per size; do not modify."""
    if (H, W) not in _pairs:
        rng = np.random.default_rng(7000 + 1000 * H + W)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        gt = np.stack([0.5 + 0.5 * np.sin(0.31 * (c + 1) * xx + 0.17 * (c + 2) * yy + c) for c in range(3)], -1).astype(np.float32)
        img = (gt + 0.05 * rng.standard_normal(gt.shape)).astype(np.float32)
        gt[:H // 3] = 1.0
        img[:H // 3] = 1.0
        img.setflags(write=False)
        gt.setflags(write=False)
        _pairs[(H, W)] = (img, gt)
    return _pairs[(H, W)]


def tensors(H, W, device="cpu"):
    """pair(H, W) as fresh torch tensors on ``device``"""
    import torch
    return tuple(torch.tensor(a, device=device) for a in pair(H, W))


_refs = {}


def reference(H, W, data_range, quantize8):
    """yardstick of pair(H, W), computed once per (size, options)"""
    key = (H, W, data_range, quantize8)
    if key not in _refs:
        _refs[key] = yardstick(*pair(H, W), data_range=data_range, quantize8=quantize8)
    return _refs[key]


def check(got_mse, got_ssim, want, what=""):
    print("%s mse %.17g (yardstick %.17g)  ssim %.17g (yardstick %.17g)" % (what, got_mse, want["mse"], got_ssim, want["ssim"]))
    assert abs(got_ssim - want["ssim"]) <= SSIM_BAR, (what, got_ssim, want["ssim"])
    assert abs(got_mse - want["mse"]) <= mse_bar(want["mse"]), (what, got_mse, want["mse"])

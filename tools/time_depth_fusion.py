#!/usr/bin/env python3
"""Times the depth-map fusion on the device and writes profiles/depth_fusion.json.

    python tools/time_depth_fusion.py [--out profiles/depth_fusion.json] [--sizes 50x400x400,100x480x640] [--torch-repeats 3]

Per size V x H x W (defaults: 50 views of 400 x 400, the NeRF-synthetic initialisation; 100 views of 480 x 640, ScanNet) on the analytic
scene of tests/depthfuse_case.py:
  kernel_ms          pnerf_depth_consistency alone (device events around the launch; pair tables already uploaded)
  consistency_ms     point_init.depth_consistency, the whole call: float64 pair tables on the host, upload, launch (host clock, synchronised)
  front_door_ms      point_init.points_from_depth_maps (filter + selection; geo_cnsst_num 2), whole call, synchronised
  torch_loop_ms      the float32 torch restatement of the reference's loop (filter_utils.py:222-259: one reprojection of ~40 element-wise
                     launches per ordered pair of views) on the same device, synchronised
  geo_agree          the share of pixels on which the two give the same geo_mask_sum (hard thresholds on two fp32 roundings)
Warm-up runs first; every figure is the median of the repeated runs, with the spread (min, max) beside it.  No GPU: it fails."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def torch_loop(depth, K, E):
    """the dense part of filter_by_masks_gpu (filter_utils.py:157-259) restated in float32 torch, statement for statement"""
    V, H, W = depth.shape
    dev = depth.device
    y_ref, x_ref = torch.meshgrid(torch.arange(0, H, device=dev), torch.arange(0, W, device=dev), indexing="ij")
    xf, yf = x_ref.reshape(-1), y_ref.reshape(-1)
    ones = torch.ones_like(xf)
    geo_all, avg_all = [], []
    for r in range(V):
        d_ref = depth[r]
        total, geo = 0, 0
        for s in range(V):
            if s == r:
                continue
            xyz_ref = torch.matmul(torch.linalg.inv(K[r]), torch.stack([xf, yf, ones], dim=0) * d_ref.reshape(-1))
            xyz_src = torch.matmul(torch.matmul(E[s], torch.linalg.inv(E[r])), torch.cat([xyz_ref, ones[None, :]], dim=0))[:3]
            k_src = torch.matmul(K[s], xyz_src)
            xy_src = k_src[:2] / k_src[2:3]
            x_src, y_src = xy_src[0].reshape(H, W), xy_src[1].reshape(H, W)
            grid = torch.stack([x_src * 2 / (W - 1) - 1, y_src * 2 / (H - 1) - 1], dim=-1)[None]
            sampled = F.grid_sample(depth[s][None, None], grid, align_corners=True, mode="bilinear", padding_mode="border")
            xyz_s = torch.matmul(torch.linalg.inv(K[s]), torch.cat([xy_src, ones[None, :]], dim=0) * sampled.reshape(-1))
            xyz_rep = torch.matmul(torch.matmul(E[r], torch.linalg.inv(E[s])), torch.cat([xyz_s, ones[None, :]], dim=0))[:3]
            d_rep = xyz_rep[2].reshape(H, W)
            k_rep = torch.matmul(K[r], xyz_rep)
            xy_rep = k_rep[:2] / k_rep[2:3]
            dist = torch.sqrt((xy_rep[0].reshape(H, W) - x_ref) ** 2 + (xy_rep[1].reshape(H, W) - y_ref) ** 2)
            rel = torch.abs(d_rep - d_ref) / d_ref
            mask = torch.logical_and(dist < 1, rel < 0.01)
            d_rep[~mask] = 0
            geo = geo + mask.to(torch.int32)
            total = total + d_rep
        geo_all.append(geo)
        avg_all.append((total + d_ref) / (geo + 1))
    return torch.stack(geo_all), torch.stack(avg_all)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), repeats=repeats)


def kernel_events(depth, K, E, warmup, repeats):
    from pointnerf_amd import _lib as L, ops, point_init
    V, H, W = depth.shape
    pairs = point_init._pair_tables(K, E).to(depth.device)
    geo = torch.empty(V, H, W, dtype=torch.int32, device=depth.device)
    avg = torch.empty(V, H, W, dtype=torch.float32, device=depth.device)
    hw = (ctypes.c_int32 * (2 * V))(*([H, W] * V))
    run = lambda: L.check(L.lib().pnerf_depth_consistency(ops._ptr(depth), hw, V, ops._ptr(pairs), ops._ptr(geo), ops._ptr(avg), ops._stream()),
                          "pnerf_depth_consistency")
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion.json"))
    ap.add_argument("--sizes", default="50x400x400,100x480x640")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_depth_fusion: no GPU (a timing without one says nothing)")
    import depthfuse_case as DC
    from pointnerf_amd import point_init
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), sizes=[])
    for size in args.sizes.split(","):
        V, H, W = (int(a) for a in size.split("x"))
        d, K, E = DC.scene(V, H, W, step_deg=360.0 / V)
        depth, K, E = (torch.from_numpy(a.astype(np.float32)).to(dev) for a in (d, K, E))
        row = dict(V=V, H=H, W=W, pairs=V * (V - 1))
        row["kernel_ms"] = kernel_events(depth, K, E, 3, args.repeats)
        row["consistency_ms"] = timed(lambda: point_init.depth_consistency(depth, K, E), 2, args.repeats)
        front = lambda: point_init.points_from_depth_maps(depth, K, E, geo_cnsst_num=2, depth_conf_thresh=0.1)
        row["front_door_ms"] = timed(front, 2, args.repeats)
        row["points_kept"] = int(front()[0].shape[0])
        row["torch_loop_ms"] = timed(lambda: torch_loop(depth, K, E), 1, args.torch_repeats)
        geo, _ = point_init.depth_consistency(depth, K, E)
        geo_t, _ = torch_loop(depth, K, E)
        row["geo_agree"] = float((geo == geo_t).float().mean())
        row["speedup_vs_torch_loop"] = row["torch_loop_ms"]["median"] / row["consistency_ms"]["median"]
        # the bytes the kernel must move at least: every map read once, 8 B written per pixel (the gathers hit the cache)
        row["kernel_min_bytes"] = V * H * W * 12
        row["kernel_GBps_of_min_bytes"] = row["kernel_min_bytes"] / (row["kernel_ms"]["median"] * 1e-3) / 1e9
        print(json.dumps(row), flush=True)
        result["sizes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

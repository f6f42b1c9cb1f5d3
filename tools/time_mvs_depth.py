#!/usr/bin/env python3
"""Times the depth estimator's stages on the device and writes profiles/mvs_depth.json.

    python tools/time_mvs_depth.py [--out profiles/mvs_depth.json] [--sizes 800x800,480x640] [--views 3] [--depths 192]

Per image size H x W (defaults: 800 x 800, the NeRF-synthetic scripts; 480 x 640), V views, D depth planes, feature maps of H/4 x W/4:
  cost_volume    pnerf_mvs_cost_volume (transpose + the fused warp-and-variance launch; device events) against the reference's formula
                 restated in float32 torch on the same device (module.py:36-70 per view, mvsnet.py:110-122), with the peak memory of both
  regress        pnerf_mvs_depth_regress (depth and confidence, no probability volume) against the torch restatement of mvsnet.py:127-136
  networks       FeatureNet on the V images and CostRegNet on the variance volume (torch's convolutions, inference form)
  whole          point_init.depth_maps_from_images for ONE reference view, whole call, synchronised (host clock)
Every stage runs in a child process of its own under `timeout`, so that a stage that hangs ends alone; the parent stops at the first stage
that fails.  Warm-up runs first; every figure is the median of 10 runs with the spread (min, max) beside it.  No GPU: it fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

STAGES = (("cost_volume", 240), ("regress", 120), ("networks", 240), ("whole", 300))      # (name, seconds allowed)


def torch_cost_volume(feats, proj, dv):
    """homo_warping per view and the variance lines, float32 torch, statement for statement (inference branch)"""
    V, C, h, w = feats.shape
    B, D = dv.shape
    dev = feats.device
    y, x = torch.meshgrid(torch.arange(0, h, dtype=torch.float32, device=dev), torch.arange(0, w, dtype=torch.float32, device=dev), indexing="ij")
    xyz = torch.stack((x.reshape(-1), y.reshape(-1), torch.ones(h * w, device=dev)))[None].repeat(B, 1, 1)
    volume_sum, volume_sq_sum = 0, 0
    for v in range(V):
        rot, trans = proj[:, v, :3, :3], proj[:, v, :3, 3:4]
        rot_depth_xyz = torch.matmul(rot, xyz).unsqueeze(2).repeat(1, 1, D, 1) * dv.view(B, 1, D, 1)
        p = rot_depth_xyz + trans.view(B, 3, 1, 1)
        xy = p[:, :2] / p[:, 2:3]
        grid = torch.stack((xy[:, 0] / ((w - 1) / 2) - 1, xy[:, 1] / ((h - 1) / 2) - 1), dim=3)
        warped = F.grid_sample(feats[v][None].expand(B, -1, -1, -1), grid.view(B, D * h, w, 2), mode="bilinear", padding_mode="zeros",
                               align_corners=False).view(B, C, D, h, w)
        volume_sum = volume_sum + warped if v == 0 else volume_sum.add_(warped)
        volume_sq_sum = volume_sq_sum + warped.pow_(2) if v == 0 else volume_sq_sum.add_(warped.pow_(2))
        del warped
    return volume_sq_sum.div_(V).sub_(volume_sum.div_(V).pow_(2))


def torch_regress(cost, dv):
    """mvsnet.py:127-136, float32 torch"""
    D = dv.shape[1]
    prob = F.softmax(cost, dim=1)
    depth = torch.sum(prob * dv.view(*dv.shape, 1, 1), 1)
    sum4 = 4 * F.avg_pool3d(F.pad(prob.unsqueeze(1), pad=(0, 0, 0, 0, 1, 2)), (4, 1, 1), stride=1, padding=0).squeeze(1)
    index = torch.sum(prob * torch.arange(D, device=cost.device, dtype=torch.float).view(D, 1, 1), 1).long()
    return depth, torch.gather(sum4, 1, index.unsqueeze(1)).squeeze(1)


def events(fn, warmup=2, repeats=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms), repeats=repeats)


def host_clock(fn, warmup=2, repeats=10):
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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del out
    return peak


def run_stage(stage, H, W, V, D):
    import mvsdepth_case as MC
    from pointnerf_amd import ops, point_init
    from pointnerf_amd.depth_estimators import MVSNet
    dev = torch.device("cuda:0")
    h, w = H // 4, W // 4
    g = torch.Generator(device="cpu").manual_seed(1)
    net = MC.fill_weights(MVSNet(), 7).to(dev)
    K = torch.tensor([[1.2 * W, 0.0, W / 2.0], [0.0, 1.2 * W, H / 2.0], [0.0, 0.0, 1.0]]).expand(V, 3, 3).clone()
    E = torch.eye(4).repeat(V, 1, 1)
    for v in range(V):
        E[v, 0, 3], E[v, 1, 3] = 0.15 * v, -0.05 * v
    proj = point_init.relative_proj_mats(K, E, list(range(V)))[None].to(dev)
    dv = point_init.depth_values_of((2.0, 6.0), D).to(dev)
    row = dict(stage=stage, H=H, W=W, V=V, D=D, h=h, w=w)
    with torch.no_grad():
        if stage == "cost_volume":
            feats = torch.randn(V, 32, h, w, generator=g).to(dev)
            row["kernel_ms"] = events(lambda: ops.mvs_cost_volume(feats, proj, dv))
            row["torch_ms"] = events(lambda: torch_cost_volume(feats, proj, dv), 1, 10)
            row["kernel_peak_MB"] = peak_mb(lambda: ops.mvs_cost_volume(feats, proj, dv))
            row["torch_peak_MB"] = peak_mb(lambda: torch_cost_volume(feats, proj, dv))
            row["volume_MB"] = 32 * D * h * w * 4 / 2 ** 20
            row["GBps_of_volume_written"] = 32 * D * h * w * 4 / (row["kernel_ms"]["median"] * 1e-3) / 1e9
            a, b = ops.mvs_cost_volume(feats, proj, dv), torch_cost_volume(feats, proj, dv)
            row["max_abs_difference"] = float((a - b).abs().max())
        elif stage == "regress":
            cost = 3.0 * torch.randn(1, D, h, w, generator=g).to(dev)
            row["kernel_ms"] = events(lambda: ops.mvs_depth_regress(cost, dv))
            row["torch_ms"] = events(lambda: torch_regress(cost, dv))
            row["kernel_peak_MB"] = peak_mb(lambda: ops.mvs_depth_regress(cost, dv))
            row["torch_peak_MB"] = peak_mb(lambda: torch_regress(cost, dv))
            row["GBps_of_logits_read"] = D * h * w * 4 / (row["kernel_ms"]["median"] * 1e-3) / 1e9
        elif stage == "networks":
            imgs = torch.rand(V, 3, H, W, generator=g).to(dev)
            var = torch.rand(1, 32, D, h, w, generator=g).to(dev)
            row["feature_net_ms"] = events(lambda: net.features_of(imgs))
            row["cost_reg_net_ms"] = events(lambda: net.cost_regularization(var), 1, 10)
            row["cost_reg_net_peak_MB"] = peak_mb(lambda: net.cost_regularization(var))
        elif stage == "whole":
            imgs = torch.rand(V, 3, H, W, generator=g).to(dev)
            whole = lambda: point_init.depth_maps_from_images(net, imgs, K, E, [list(range(V))], (2.0, 6.0), n_depth=D)
            row["per_view_ms"] = host_clock(whole, 1, 10)
            row["peak_MB"] = peak_mb(whole)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvs_depth.json"))
    ap.add_argument("--sizes", default="800x800,480x640")
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--depths", type=int, default=192)
    ap.add_argument("--stage", default=None, help="run one stage in this process and print its JSON row (what the parent starts)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mvs_depth: no GPU (a timing without one says nothing)")
    if args.stage:
        H, W = (int(a) for a in args.sizes.split("x"))
        print("ROW " + json.dumps(run_stage(args.stage, H, W, args.views, args.depths)), flush=True)
        return
    result = dict(device=torch.cuda.get_device_name(0), rows=[])
    for size in args.sizes.split(","):
        for stage, limit in STAGES:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--stage", stage, "--sizes", size,
                   "--views", str(args.views), "--depths", str(args.depths)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            rows = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
            if p.returncode != 0 or not rows:
                sys.stderr.write(p.stdout[-4000:])
                raise SystemExit("time_mvs_depth: stage %s at %s ended with status %d; nothing further is started" % (stage, size, p.returncode))
            print(rows[0], flush=True)
            result["rows"].append(json.loads(rows[0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

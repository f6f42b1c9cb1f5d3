#!/usr/bin/env python3
"""Times the route from an external cloud to per-view point groups on the device and writes profiles/cloud_init.json.

    python tools/time_cloud_init.py [--out profiles/cloud_init.json] [--points 2000000,20000000] [--cameras 100,300] [--route-points 2000000]

nearest_view, per (N points, M cameras) (defaults: the bench's lego and barn sizes, 2 M and 20 M points; 100 and 300 cameras on a ring):
  kernel_ms            pnerf_nearest_view alone (device events around the launch)
  call_ms              point_init.nearest_view, the whole call with its int64 [N,1] result (host clock, synchronised)
  torch_10000_ms       the reference's loop (run/train_ft.py:39-48) restated in float32 torch on the same device in its own 10 000-point
                       slices, synchronised
  torch_big_ms         the same statements in the largest slices whose [slice, M, 3] temporaries stay below 2 GiB each: the comparison
                       without the launch overhead of thousands of small slices
  agree                the share of points on which kernel and torch loop name the same camera (an argmin over two fp32 roundings)
The whole route, at --route-points points (70 % in a first cloud, 30 % in a second one that is wider; merge at 100, crop, no down-sampling,
300 cameras):
  route_ms             point_init.points_from_cloud, whole call, synchronised
  torch_route_ms       run/train_ft.py:657-669, 675-680, 707-710 restated in float32 torch (torch.unique(dim=0) twice, the mask volume, the
                       10 000-point nearest_view loop, one boolean index per view)
  points_in_another_group_than_torch   half the summed difference of the group sizes over the points: a lower bound of the share of points the two
                       send to different views (near-ties of the argmin; merge and crop keep the same points)
Warm-up runs first; every figure is the median of the repeated runs, with the spread (min, max) beside it.  No GPU: it fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def torch_nearest_view(campos, raydir, xyz, step=10000):
    """run/train_ft.py:39-48, statement for statement"""
    cam_ind = torch.zeros([0, 1], device=campos.device, dtype=torch.long)
    for i in range(0, len(xyz), step):
        dists = xyz[i:min(len(xyz), i + step), None, :] - campos[None, ...]
        dists_norm = torch.norm(dists, dim=-1)
        dists_dir = dists / (dists_norm[..., None] + 1e-6)
        dists = dists_norm / 200 + (1.1 - torch.sum(dists_dir * raydir[None, :], dim=-1))
        cam_ind = torch.cat([cam_ind, torch.argmin(dists, dim=1).view(-1, 1)], dim=0)
    return cam_ind


def torch_vox_ind(xyz, vox_res, space_min=None, space_max=None):
    """models/mvs/mvs_utils.py:520-534"""
    if space_min is None:
        xyz_min, xyz_max = torch.min(xyz, dim=-2)[0], torch.max(xyz, dim=-2)[0]
        space_edge = torch.max(xyz_max - xyz_min) * 1.05
        xyz_mid = (xyz_max + xyz_min) / 2
        space_min = xyz_mid - space_edge / 2
        space_max = xyz_mid + space_edge / 2
    else:
        space_edge = space_max - space_min
    construct_vox_sz = space_edge / vox_res
    xyz_shift = xyz - space_min[None, ...]
    sparse_grid_idx, inv_idx = torch.unique(torch.floor(xyz_shift / construct_vox_sz[None, ...]).to(torch.int32), dim=0, return_inverse=True)
    return sparse_grid_idx, inv_idx, space_min, space_max


def torch_route(a, b, campos, camdir, ranges, filter_res=100):
    """run/train_ft.py:657-669 (merge), :672 (concatenate), :675-680 (crop), :707-710 (nearest view and the per-view lists)"""
    pc_grid_id, _, pc_space_min, pc_space_max = torch_vox_ind(a, filter_res)
    d_grid_id, depth_inds, _, _ = torch_vox_ind(b, filter_res, space_min=pc_space_min, space_max=pc_space_max)
    all_grid = torch.cat([pc_grid_id, d_grid_id], dim=0)
    min_id = torch.min(all_grid, dim=-2)[0]
    max_id = torch.max(all_grid, dim=-2)[0] - min_id
    mask = torch.ones((max_id + 1).cpu().numpy().tolist(), device=d_grid_id.device)
    pc_maskgrid_id = (pc_grid_id - min_id[None, ...]).to(torch.long)
    mask[pc_maskgrid_id[..., 0], pc_maskgrid_id[..., 1], pc_maskgrid_id[..., 2]] = 0
    depth_maskinds = (d_grid_id[depth_inds, :] - min_id).to(torch.long)
    depth_maskinds = mask[depth_maskinds[..., 0], depth_maskinds[..., 1], depth_maskinds[..., 2]]
    pts = torch.cat([a, b[depth_maskinds > 0]], dim=0)
    rng = torch.as_tensor(ranges, device=pts.device, dtype=torch.float32)
    pts = pts[torch.prod(torch.logical_and(pts[..., :3] >= rng[None, :3], pts[..., :3] <= rng[None, 3:]), dim=-1) > 0]
    cam_ind = torch_nearest_view(campos, camdir, pts)
    unique_cam_ind = torch.unique(cam_ind)
    return [pts[cam_ind[:, 0] == unique_cam_ind[i], :] for i in range(len(unique_cam_ind))], unique_cam_ind


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


def kernel_events(xyz, campos, camdir, warmup, repeats):
    from pointnerf_amd import _lib as L, ops
    cam = torch.empty(len(xyz), dtype=torch.int32, device=xyz.device)
    run = lambda: L.check(L.lib().pnerf_nearest_view(ops._ptr(xyz), len(xyz), ops._ptr(campos), ops._ptr(camdir), len(campos), ops._ptr(cam),
                                                     ops._stream()), "pnerf_nearest_view")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_init.json"))
    ap.add_argument("--points", default="2000000,20000000")
    ap.add_argument("--cameras", default="100,300")
    ap.add_argument("--route-points", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--torch-repeats", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cloud_init: no GPU (a timing without one says nothing)")
    import cloudinit_case as CC
    from pointnerf_amd import point_init
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(0), nearest_view=[], route=None)
    gen = torch.Generator(device="cpu").manual_seed(7)
    for n in (int(a) for a in args.points.split(",")):
        xyz = ((torch.rand(n, 3, generator=gen) * 2 - 1) * 1.2).to(dev)
        for M in (int(a) for a in args.cameras.split(",")):
            campos, camdir = (torch.from_numpy(a).to(dev) for a in CC.cameras("ring", M))
            row = dict(N=n, M=M, pairs=n * M)
            row["kernel_ms"] = kernel_events(xyz, campos, camdir, 2, args.repeats)
            row["call_ms"] = timed(lambda: point_init.nearest_view(campos, camdir, xyz), 1, args.repeats)
            row["torch_10000_ms"] = timed(lambda: torch_nearest_view(campos, camdir, xyz), 1, args.torch_repeats)
            big = max(10000, (2 << 30) // (12 * M))
            row["big_slice"] = min(big, n)
            row["torch_big_ms"] = timed(lambda: torch_nearest_view(campos, camdir, xyz, big), 1, args.torch_repeats)
            row["agree"] = float((point_init.nearest_view(campos, camdir, xyz) == torch_nearest_view(campos, camdir, xyz, big)).float().mean())
            row["speedup_vs_torch_10000"] = row["torch_10000_ms"]["median"] / row["call_ms"]["median"]
            row["speedup_vs_torch_big"] = row["torch_big_ms"]["median"] / row["call_ms"]["median"]
            row["kernel_pairs_per_s"] = row["pairs"] / (row["kernel_ms"]["median"] * 1e-3)
            print(json.dumps(row), flush=True)
            result["nearest_view"].append(row)
        del xyz
        torch.cuda.empty_cache()
    n = args.route_points
    na = int(0.7 * n)
    a = ((torch.rand(na, 3, generator=gen) * 2 - 1) * 1.0).to(dev)
    b = ((torch.rand(n - na, 3, generator=gen) * 2 - 1) * 1.3).to(dev)
    campos, camdir = (torch.from_numpy(x).to(dev) for x in CC.cameras("ring", 300))
    ranges = [-1.2, -1.2, -1.1, 1.2, 1.2, 1.2]
    row = dict(N=n, M=300, merge_res=100, ranges=ranges)
    route = lambda: point_init.points_from_cloud([a, b], campos, camdir, vox_res=0, ranges=ranges, merge_res=100)
    row["route_ms"] = timed(route, 1, args.repeats)
    row["torch_route_ms"] = timed(lambda: torch_route(a, b, campos, camdir, ranges), 1, args.torch_repeats)
    xyz, ids, off, _ = route()
    lists, uniq = torch_route(a, b, campos, camdir, ranges)
    row["points_out"], row["groups"] = int(len(xyz)), int(len(ids))
    row["same_points_and_groups_as_torch"] = bool(len(xyz) == sum(len(x) for x in lists) and torch.equal(ids, uniq))
    sizes = torch.tensor([len(x) for x in lists], device=dev)
    row["points_in_another_group_than_torch"] = float((off[1:] - off[:-1] - sizes).abs().sum()) / 2 / max(len(xyz), 1) if torch.equal(ids, uniq) else None
    row["speedup_vs_torch_route"] = row["torch_route_ms"]["median"] / row["route_ms"]["median"]
    print(json.dumps(row), flush=True)
    result["route"] = row
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

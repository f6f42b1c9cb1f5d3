"""Time one training step of a bench configuration with and without xyz_grad (trainable point positions), and split it by kernel.

    python tools/time_xyz_grad.py [--config lego] [--rays 65536] [--steps 10] [--warmup 3]

Both runs build the model of bench.py (same points, weights and ray batches) and time forward + backward + the two FusedAdam steps with
CUDA events; the per-kernel split comes from the library's profiling scopes (pnerf_prof_*), collected over the timed steps.  With
xyz_grad the step also pays a voxel-grid rebuild: the optimiser moves the points, which drops the grid cache.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from pointnerf_amd import ops  # noqa: E402
from pointnerf_amd.optim import FusedAdam  # noqa: E402


def run(cfg, rays, steps, warmup, xyz_grad):
    _, opt_fn, points_fn, n_points, rays_fn = bench._cfg()[cfg]
    opt = opt_fn(xyz_grad=xyz_grad)
    dev = torch.device("cuda:0")
    model = bench.build_model(opt, n_points, dev, points_fn)
    npnt, agg = model.neural_points, model.aggregator
    pts = [npnt.points_embeding, npnt.points_conf, npnt.points_dir, npnt.points_color] + ([npnt.xyz] if xyz_grad else [])
    o_mlp = FusedAdam([p for p in agg.parameters() if p.requires_grad], lr=opt.lr, betas=(0.9, 0.999))
    o_pts = FusedAdam(pts, lr=opt.plr, betas=(0.9, 0.999))
    times = []
    for i in range(warmup + steps):
        inp = bench.step_inputs(i, 0, 1, rays, dev, rays_fn)
        if i == warmup:
            torch.cuda.synchronize()
            ops.prof_enable(True)
            ops.prof_collect()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        o_mlp.zero_grad(set_to_none=True); o_pts.zero_grad(set_to_none=True)
        out = model(**inp)
        bench.loss_fn(opt, out, inp, 1).backward()
        o_mlp.step(); o_pts.step()
        t1.record()
        if i >= warmup:
            times.append((t0, t1))
    torch.cuda.synchronize()
    kern = {k: round(v[0] / steps, 4) for k, v in ops.prof_collect().items() if v[1] > 0}
    ops.prof_enable(False)
    ms = sorted(a.elapsed_time(b) for a, b in times)
    assert not xyz_grad or npnt.xyz.grad is not None
    return dict(step_ms_median=ms[len(ms) // 2], step_ms_min=ms[0], kernels_ms_per_step=kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="lego", choices=sorted(bench.CONFIGS))
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"config": a.config, "rays": a.rays}
    for xg in (0, 1):
        res["xyz_grad=%d" % xg] = run(a.config, a.rays, a.steps, a.warmup, xg)
    res["ratio"] = res["xyz_grad=1"]["step_ms_median"] / res["xyz_grad=0"]["step_ms_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

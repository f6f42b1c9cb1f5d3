#!/usr/bin/env python3
"""What per-point Rw2c frames (scene editing: pnerf_points.frames, the FRAMES instances of k_agg_forward / k_color_forward) cost a render: on
the GPU, after a warm-up, times (HIP events) eval_loop.render_image of ONE 800 x 800 view (640 000 rays, the default chunk of 160 000) of the
`chair` bench scene (BASELINE.json configs[0]: bench.py --config chair) with one frame per point (three parts, assigned at random) and with
the one uniform frame every other render uses.  The two are timed in alternating rounds of `--iters` images each, one event pair per round;
prints ONE JSON line with the median and the minimum per image over the rounds and their ratio.  Before timing it checks that per-point
IDENTITY frames give the uniform image bit for bit.  No pass / fail ratio: the number is a measurement.  Needs a GPU.

    python tools/time_editing_render.py [--rounds 7] [--iters 4]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from pointnerf_amd import config, eval_loop, scenes


def frames_of_parts(n, parts=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    rots = [torch.eye(3)]
    for _ in range(parts - 1):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        rots.append(q * torch.sign(torch.det(q)))
    return torch.stack(rots)[torch.randint(0, parts, (n,), generator=g)].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=4)          # an image takes tens of milliseconds: 4 make a window of 0.1-0.3 s
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_editing_render.py: no GPU (a timing on anything else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    H = W = 800
    opt = config.chair_opt()
    model = bench.build_model(opt, 8192, dev, points_fn=scenes.chair_points)
    npnt = model.neural_points
    n = npnt.xyz.shape[0]
    d = scenes.block_rays(theta_deg=30.0, x0=0, y0=0, size=4)                   # the camera of the bench view
    cam = {k: torch.from_numpy(np.ascontiguousarray(d[k])).to(dev) for k in ("campos", "camrotc2w", "intrinsic", "near", "far", "bg_color")}
    tensors = (npnt.xyz.detach(), npnt.points_embeding.detach())
    kw = dict(points_color=npnt.points_color.detach(), points_dir=npnt.points_dir.detach(), points_conf=npnt.points_conf.detach())

    npnt.editing_set_points(*tensors, **kw)                       # plain tensors, as a composed scene holds them; the voxel grid is built once
    eye = npnt.Rw2c

    def render(frames):
        npnt.Rw2c = eye if frames is None else frames             # [3,3]: the uniform path; [N,3,3]: pnerf_points.frames
        return eval_loop.render_image(model, cam["campos"], cam["camrotc2w"], cam["intrinsic"][0], H, W, cam["near"], cam["far"], cam["bg_color"])

    per_point = frames_of_parts(n).to(dev)
    img_u, hit = render(None)
    img_i, _ = render(torch.eye(3, device=dev)[None].repeat(n, 1, 1))
    if not torch.equal(img_u, img_i):
        raise SystemExit("time_editing_render.py: per-point identity frames do not give the uniform image")
    img_f, _ = render(per_point)
    moved = float((img_f - img_u).abs().max())

    def timed(frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            render(frames)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for _ in range(2):                                             # warm-up of every shape the timed window uses
        render(per_point); render(None)
    torch.cuda.synchronize()
    t = {True: [], False: []}
    for _ in range(args.rounds):
        t[True].append(timed(per_point))
        t[False].append(timed(None))
    res = dict(view="%dx%d" % (H, W), scene="chair (%d points, K=%d, SR=%d)" % (n, opt.K, opt.SR), chunk=160000, rounds=args.rounds,
               images_per_round=args.iters, rays_hit=int(hit.sum()),
               frames_ms_median=float(np.median(t[True])), frames_ms_min=float(np.min(t[True])),
               uniform_ms_median=float(np.median(t[False])), uniform_ms_min=float(np.min(t[False])),
               image_max_abs_change=moved, device=torch.cuda.get_device_name(0))
    res["frames_over_uniform"] = res["frames_ms_median"] / res["uniform_ms_median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the evaluation scorer costs next to the render it scores: on the GPU, after a warm-up, times (HIP events) the scoring of one
800 x 800 image pair (eval_loop.image_scores: pnerf_image_metrics + the few device scalar operations behind psnr / ssim / rmse) and, in the
same run, eval_loop.render_image of an 800 x 800 view of the `chair` bench scene (BASELINE.json configs[0]: bench.py --config chair).
The two are timed in alternating rounds of `--iters` calls each, one event pair per round; prints ONE JSON line with the median and the
minimum per call over the rounds.  Needs a GPU: there is nothing to time without one.

    python tools/time_image_metrics.py [--rounds 7] [--iters 20]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_metrics.py: no GPU (a timing on anything else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    H = W = 800
    opt = config.chair_opt(is_train=0)
    model = bench.build_model(opt, 8192, dev, points_fn=scenes.chair_points)
    d0 = scenes.block_rays(theta_deg=30.0, size=1)
    cam = {k: torch.from_numpy(np.ascontiguousarray(d0[k])).to(dev) for k in ("campos", "camrotc2w", "near", "far", "bg_color")}
    intr = torch.from_numpy(np.asarray(scenes.synth_camera(30.0)[1], dtype=np.float32)).to(dev)

    def render():
        return eval_loop.render_image(model, cam["campos"], cam["camrotc2w"], intr, H, W, cam["near"], cam["far"], cam["bg_color"])

    img, hit = render()
    img = img.contiguous()
    torch.manual_seed(0)
    gt = (img + 0.05 * torch.randn_like(img)).contiguous()         # a ground truth the render is close to, like a trained model's

    def score():
        return eval_loop.image_scores(img, gt)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for _ in range(3):                                             # warm-up of every shape the timed window uses
        render(); score()
    torch.cuda.synchronize()
    t_score, t_render = [], []
    for _ in range(args.rounds):
        t_score.append(timed(score))
        t_render.append(timed(render))
    s = {k: float(v) for k, v in score().items()}
    res = dict(image="%dx%d" % (H, W), scene="chair (8192 points, K=4, SR=32)", rounds=args.rounds, calls_per_round=args.iters,
               score_ms_median=float(np.median(t_score)), score_ms_min=float(np.min(t_score)),
               render_ms_median=float(np.median(t_render)), render_ms_min=float(np.min(t_render)),
               rays_hit=int(hit.sum()), scores=s, device=torch.cuda.get_device_name(0))
    res["score_over_render"] = res["score_ms_median"] / res["render_ms_median"]
    print(json.dumps(res))
    if not res["score_ms_median"] < res["render_ms_median"]:
        raise SystemExit("time_image_metrics.py: scoring the image (%.3f ms) is not cheaper than rendering it (%.3f ms)"
                         % (res["score_ms_median"], res["render_ms_median"]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the probe pass of the point-growing step costs with and without the fused probe kernels: on the GPU, after a warm-up, times (HIP
events) probe.probe_hole on ONE 800 x 800 view (640 000 rays, the default chunk of 160 000) of the `chair` bench scene (BASELINE.json
configs[0]: bench.py --config chair) with ``fused=True`` (pnerf_probe_rays + pnerf_probe_hole_mask + the existing compaction) and with
``fused=False`` (the reference's compacted shapes through ATen: the baseline, the code as it was before the fused pass existed).  The two are
timed in alternating rounds of `--iters` calls each, one event pair per round; prints ONE JSON line with the median and the minimum per
view over the rounds, the number of candidates (equal in both forms, checked) and the number of synchronising torch calls per view that
torch's sync debug mode reports for each form.  Fails if the fused pass is not the faster of the two.  Needs a GPU: there is nothing to
time without one.

    python tools/time_probe_pass.py [--rounds 7] [--iters 40]
"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from pointnerf_amd import config, probe, scenes
from pointnerf_amd.neural_points_volumetric_model import fill_invalid


class Shell:
    """what probe_hole needs of the model shell (device, opt, the ray marcher, set_input, test) around the bench's bare ray marcher"""

    def __init__(self, marcher, opt, dev):
        self.net_ray_marching, self.opt, self.device = marcher, opt, dev

    def set_input(self, data):
        self.input = {k: (v.to(self.device) if isinstance(v, torch.Tensor) else v) for k, v in data.items()}

    def test(self):
        with torch.no_grad():
            raw = self.net_ray_marching(**{k: v for k, v in self.input.items() if k != "id"})
            return fill_invalid(raw, self.input.get("bg_color"), prob=getattr(self.opt, "prob", 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)        # a view takes milliseconds: 40 make a window of 0.1-0.2 s
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_probe_pass.py: no GPU (a timing on anything else says nothing about the MI355X)")
    dev = torch.device("cuda:0")
    H = W = 800
    opt = config.chair_opt(**config.model_shell_flags(is_train=0, prob_num_step=1))
    model = Shell(bench.build_model(opt, 8192, dev, points_fn=scenes.chair_points), opt, dev)
    d = scenes.block_rays(theta_deg=30.0, x0=0, y0=0, size=H)                      # the whole view, row-major, random ground truth
    view = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items() if k not in ("h", "w")}
    view["id"] = 0

    state = {}

    def run(fused, thresh, keep=None):
        out = probe.probe_hole(model, [view], opt, H, W, test_steps=0, opacity_thresh=thresh, frame_ids=[0], fused=fused,
                               on_view=(lambda i, maps, m: state.__setitem__(keep, (maps["ray_max_shading_opacity"].clone(), maps["ray_mask"].clone(), m)))
                               if keep else None)
        return out

    # the threshold: the median of the rendered maxima over the rays that hit (a random-init MLP renders opacities of ~1e-3: the scripts' 0.7
    # would select nothing and the gathers of the candidates would not be part of what is timed)
    run(False, 0.0, keep="first")
    op, mask, _ = state["first"]
    thresh = float(op[..., 0][mask[..., 0] > 0].median())
    n = {f: int(run(f, thresh)[0].shape[0]) for f in (True, False)}
    if n[True] != n[False] or n[True] == 0:
        raise SystemExit("time_probe_pass.py: %d fused and %d unfused candidates" % (n[True], n[False]))

    def timed(fused):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            run(fused, thresh)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for _ in range(2):                                             # warm-up of every shape the timed window uses
        run(True, thresh); run(False, thresh)
    torch.cuda.synchronize()
    t = {True: [], False: []}
    for _ in range(args.rounds):
        t[True].append(timed(True))
        t[False].append(timed(False))

    def syncs(fused):                                              # synchronising torch calls of one view (torch.cuda sync debug mode)
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                run(fused, thresh)
            return sum("synchroniz" in str(w.message).lower() for w in rec)
        finally:
            torch.cuda.set_sync_debug_mode("default")

    res = dict(view="%dx%d" % (H, W), scene="chair (8192 points, K=4, SR=32)", chunk=160000, rounds=args.rounds, views_per_round=args.iters,
               fused_ms_median=float(np.median(t[True])), fused_ms_min=float(np.min(t[True])),
               unfused_ms_median=float(np.median(t[False])), unfused_ms_min=float(np.min(t[False])),
               rays_hit=int((mask > 0).sum()), candidates=n[True], opacity_thresh=thresh,
               host_syncs_per_view_fused=syncs(True), host_syncs_per_view_unfused=syncs(False), device=torch.cuda.get_device_name(0))
    res["unfused_over_fused"] = res["unfused_ms_median"] / res["fused_ms_median"]
    print(json.dumps(res))
    if not res["fused_ms_median"] < res["unfused_ms_median"]:
        raise SystemExit("time_probe_pass.py: the fused probe pass (%.3f ms) is not faster than the unfused one (%.3f ms)"
                         % (res["fused_ms_median"], res["unfused_ms_median"]))


if __name__ == "__main__":
    main()

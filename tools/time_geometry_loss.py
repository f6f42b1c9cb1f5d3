"""Time one training step of the configs[1] benchmark step (lego, 65 536 rays) with the depth and bg losses on (geometry_grad, DESIGN.md
4.10) and with them off, in one process, and -- optionally -- the step with the losses off against another build of the library.

    python tools/time_geometry_loss.py [--rounds 9] [--warmup 3] [--ab-tree DIR] [--out profiles/geometry_loss.json]

The parent process never touches the GPU: the measurement runs in one child under `timeout`.  The child builds bench.py's model (same points,
weights and ray batches; the fused colour and zero-one losses as bench.py sets them), warms both variants up on every batch of the timed
window, then times whole steps (zero_grad, forward, loss, backward, the two FusedAdam steps) with device events in ALTERNATING rounds
(off, on, off, on, ...), every round on the same ray batch for both, and reports the two medians, the off variant's own round-to-round
spread (max - min) and the per-kernel split of each variant from the library's profiling scopes, taken in one more step each after the
timed rounds.  What the losses add: one k_ray_geometry pass (24 bytes per slot), the two per-ray kernels of the loss pass, and the GEOM
instance of the ray march's backward in the place of the plain one.  No time bar is set in advance; the JSON carries every figure.

--ab-tree DIR: a checkout of ANOTHER commit (the parent's) with its library built.  `bench.py --gpus 1 --no-variants --cpu-rays 0` is then
run in that tree and in this one, alternating (A B A B ...: the A/B of library builds of tools/gpu_ab_lib.sh, each side with its own
binding), and the step times of both, their difference and the spread of the repeats of ONE side go into the JSON under "ab"."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_DEPTH, W_BG = 0.1, 0.1


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from pointnerf_amd import losses, ops
    from pointnerf_amd.optim import FusedAdam

    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    _, opt_fn, points_fn, n_points, rays_fn = bench._cfg()["lego"]
    opt = opt_fn(is_train=1)
    model = bench.build_model(opt, n_points, dev, points_fn)
    model.fused_zero_one = model.fused_color_loss = True
    npnt, agg = model.neural_points, model.aggregator
    o_mlp = FusedAdam([p for p in agg.parameters() if p.requires_grad], lr=opt.lr, betas=(0.9, 0.999))
    o_pts = FusedAdam([npnt.points_embeding, npnt.points_conf, npnt.points_dir, npnt.points_color], lr=opt.plr, betas=(0.9, 0.999))
    gen = torch.Generator().manual_seed(0)
    gt_depth = (2.0 + 4.0 * torch.rand(1, a.rays, 1, generator=gen)).to(dev)
    gt_mask = (torch.rand(1, a.rays, 1, generator=gen) < 0.6).float().to(dev)
    batches = [bench.step_inputs(i, 0, 1, a.rays, dev, rays_fn) for i in range(a.rounds)]

    def step(inp, on):
        model.geometry_grad = bool(on)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o_mlp.zero_grad(set_to_none=True); o_pts.zero_grad(set_to_none=True)
        out = model(**inp)
        loss = bench.loss_fn(opt, out, inp, 1)
        if on:
            loss = loss + W_DEPTH * losses.depth(out, gt_depth, gt_mask)[0] / a.rays + W_BG * losses.background(out, gt_mask)[0] / a.rays
        loss.backward()
        o_mlp.step(); o_pts.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), float(loss.detach())

    for _ in range(a.warmup):
        for inp in batches:
            step(inp, False); step(inp, True)
    off, on = [], []
    for inp in batches:
        off.append(step(inp, False)[0])
        on.append(step(inp, True)[0])
    kern = {}
    for name, flag in (("off", False), ("on", True)):
        ops.prof_enable(True)
        ops.prof_collect()
        _, last = step(batches[0], flag)
        kern[name] = {k: round(v[0], 4) for k, v in ops.prof_collect().items() if v[1] > 0}
        ops.prof_enable(False)
        assert last == last, "the loss is not finite"
    model.geometry_grad = False
    med = lambda v: sorted(v)[len(v) // 2]
    res = dict(config="lego", rays=a.rays, K=int(opt.K), SR=int(opt.SR), rounds=a.rounds, warmup=a.warmup,
               valid_samples=int(model.last_stats["n_valid_samples"]), rays_hit=int(model.last_stats["rays_hit"]),
               off_ms_median=round(med(off), 4), on_ms_median=round(med(on), 4), off_ms=[round(x, 4) for x in off], on_ms=[round(x, 4) for x in on],
               off_spread_ms=round(max(off) - min(off), 4), kernels_ms_one_step=kern)
    res["extra_ms"] = round(res["on_ms_median"] - res["off_ms_median"], 4)
    res["extra_share"] = round(res["extra_ms"] / res["off_ms_median"], 5)
    print(json.dumps(res))
    return res


def bench_step_ms(tree, steps, warmup, timeout):
    """step time of `bench.py --gpus 1` run in ``tree`` (a process of its own), from its JSON result line"""
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-variants",
           "--cpu-rays", "0", "--no-prof"]
    out = subprocess.run(cmd, cwd=tree, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    if out.returncode != 0:
        raise SystemExit("time_geometry_loss: bench.py in %s ended with status %d" % (tree, out.returncode))
    for line in reversed(out.stdout.decode().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            for key in ("step_ms", "ms_per_step", "step_ms_median"):
                if key in r:
                    return float(r[key])
            return 1e3 * float(r["rays"]) / float(r["value"]) if "value" in r and "rays" in r else float("nan")
    raise SystemExit("time_geometry_loss: no JSON line from bench.py in %s" % tree)


def ab(a):
    """this tree (B) against ``--ab-tree`` (A), alternating; the spread is that of the repeats of each side"""
    A, B = [], []
    for _ in range(a.ab_repeats):
        A.append(bench_step_ms(a.ab_tree, a.ab_steps, a.warmup, a.timeout))
        B.append(bench_step_ms(ROOT, a.ab_steps, a.warmup, a.timeout))
    med = lambda v: sorted(v)[len(v) // 2]
    spread = max(max(A) - min(A), max(B) - min(B))
    res = dict(other_tree_step_ms=[round(x, 4) for x in A], this_tree_step_ms=[round(x, 4) for x in B], other_median=round(med(A), 4),
               this_median=round(med(B), 4), difference_ms=round(med(B) - med(A), 4), run_to_run_spread_ms=round(spread, 4))
    res["inside_spread"] = bool(abs(res["difference_ms"]) <= res["run_to_run_spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts)")
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--ab-tree", default=None, help="a checkout of another commit with its library built: A/B of bench.py's step, losses off")
    ap.add_argument("--ab-repeats", type=int, default=3)
    ap.add_argument("--ab-steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_loss.json"))
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rays", str(a.rays), "--rounds", str(a.rounds),
           "--warmup", str(a.warmup)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE)
    if out.returncode != 0:
        raise SystemExit("time_geometry_loss: the measurement ended with status %d" % out.returncode)
    res = json.loads([l for l in out.stdout.decode().splitlines() if l.startswith("{")][-1])
    if a.ab_tree:
        res["ab"] = ab(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

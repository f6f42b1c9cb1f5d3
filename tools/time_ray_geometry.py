"""Time eval_loop.render_image of an 800 x 800 view of the bench's `chair` scene with the depth and opacity maps (geometry=True:
NeuralPointsRayMarching.ray_geometry) against the same render without them (geometry=False), in the same process.

    python tools/time_ray_geometry.py [--rounds 9] [--warmup 3] [--out profiles/ray_geometry.json]

The parent process never touches the GPU: the measurement runs in one child under `timeout`.  The child warms both renders up, then times
them in ALTERNATING rounds (plain, geometry, plain, geometry, ...) with device events around each whole render_image call, and reports the
two medians, the plain render's own round-to-round spread (max - min over its rounds) and the time of one k_raymarch_forward launch, measured
in the same run by the library's event pairs around that launch (ops.prof_enable / prof_collect) during one more plain render.  The one
assertion: the geometry render's median exceeds the plain one's by less than that spread plus that launch time -- the new pass reads fewer
bytes per sample than the ray march (24 against ~44), so one ray-march launch is the yardstick for what it may cost.  No threshold is set
in advance; the JSON line carries every figure."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 800


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from pointnerf_amd import eval_loop, ops, scenes

    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    _, opt_fn, points_fn, n_points, _ = bench._cfg()["chair"]
    opt = opt_fn(is_train=0)
    model = bench.build_model(opt, n_points, dev, points_fn)
    d = scenes.block_rays(theta_deg=30.0, size=1)                      # the pose of configs[0]; only its camera is used
    t = lambda x: torch.from_numpy(x).to(dev)
    args = (model, t(d["campos"]), t(d["camrotc2w"]), t(d["intrinsic"][0]), SIZE, SIZE, t(d["near"]), t(d["far"]), t(d["bg_color"]))

    def timed(geometry):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = eval_loop.render_image(*args, chunk=a.chunk, geometry=geometry)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for _ in range(a.warmup):
        timed(False); timed(True)
    plain, geo = [], []
    for _ in range(a.rounds):
        plain.append(timed(False)[0])
        geo.append(timed(True)[0])
    _, (img0, hit0) = timed(False)
    _, (img1, hit1, maps) = timed(True)
    assert torch.equal(img0, img1) and torch.equal(hit0, hit1) and model.ray_geometry is False
    ops.prof_enable(True)
    ops.prof_collect()
    eval_loop.render_image(*args, chunk=a.chunk)
    prof = ops.prof_collect()
    ops.prof_enable(False)
    rm_ms, rm_n = prof["raymarch_forward"]
    assert rm_n == (SIZE * SIZE + a.chunk - 1) // a.chunk, rm_n
    med = lambda v: sorted(v)[len(v) // 2]
    res = dict(scene="chair", view=[SIZE, SIZE], chunk=a.chunk, rounds=a.rounds, warmup=a.warmup, K=int(opt.K), SR=int(opt.SR),
               hit_rays=int(hit0.sum()), plain_ms_median=round(med(plain), 4), geometry_ms_median=round(med(geo), 4),
               plain_ms=[round(x, 4) for x in plain], geometry_ms=[round(x, 4) for x in geo],
               plain_spread_ms=round(max(plain) - min(plain), 4), raymarch_forward_launches=int(rm_n), raymarch_forward_ms_per_launch=round(rm_ms / rm_n, 4),
               depth_of_hit_rays=[float(maps["depth"][maps["acc"] > 0].min()), float(maps["depth"].max())] if int(hit0.sum()) else None)
    res["extra_ms"] = round(res["geometry_ms_median"] - res["plain_ms_median"], 4)
    res["allowed_ms"] = round(res["plain_spread_ms"] + res["raymarch_forward_ms_per_launch"], 4)
    res["within"] = bool(res["extra_ms"] < res["allowed_ms"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert res["within"], "geometry=True costs %.4f ms more than the plain render; allowed %.4f ms" % (res["extra_ms"], res["allowed_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=160000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_geometry.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--warmup", str(a.warmup),
           "--chunk", str(a.chunk), "--out", a.out]
    rc = subprocess.call(cmd)
    if rc != 0:
        raise SystemExit("time_ray_geometry: the measurement ended with status %d" % rc)


if __name__ == "__main__":
    main()

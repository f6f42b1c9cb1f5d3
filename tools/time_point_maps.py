"""Time the point attribute maps, the pick and the lifting (ops.ray_attributes / ops.lift_to_points, pointnerf_amd/point_maps.py)
against the render they sit behind, in one process.

    python tools/time_point_maps.py [--rounds 9] [--warmup 3] [--out profiles/point_maps.json]

Two settings: (a) the 800 x 800 view of the bench's `chair` scene (host-bound: few rays hit), where eval_loop.render_image, the plain
render_dense chunks and the two module functions render_point_maps / lift_image are timed end to end; (b) two chunks of 160 000 random rays of
the bench's lego configuration, where the plain render_dense of a chunk and the two ops ALONE on that chunk's dense tensors are timed
(ray_attributes at C = 0, 1, 3, 32; lift_to_points at C = 0, 3; the random rays are no pixel grid, so the module functions do not apply there).

The parent process never touches the GPU: the measurement runs in one child under `timeout`.  After a warm-up every item is timed once per
round, the items ALTERNATING within a round, with device events around it (the small ops: around `--inner` back-to-back calls, divided).  Per
op the report carries the algorithmic bytes (blend_w of the hit rays, weight / sample_pidx of their samples with blend_w != 0, one table row
per entry with g != 0, the outputs) and the rate they are moved at; for the lift also the ADDED bytes ((C + 1) words per entry with g != 0)
per second beside the ~1.3 TB/s that float atomics reach chip-wide.  Nothing is a target.  The one assertion: on each lego chunk
ray_attributes at C = 3 plus the render's own round-to-round spread stays below the plain render of that chunk."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 800
LEGO_RAYS = 160000
ATOMIC_GUIDE_TBS = 1.3


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from pointnerf_amd import eval_loop, ops, point_maps, scenes

    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]

    def timed(fn, inner=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def rounds(items):
        """items: {name: (fn, inner)} -> {name: [ms per round]}, the items alternating within every round"""
        for _ in range(a.warmup):
            for fn, inner in items.values():
                timed(fn, inner)
        ms = {k: [] for k in items}
        for _ in range(a.rounds):
            for k, (fn, inner) in items.items():
                ms[k].append(timed(fn, inner))
        return ms

    def summary(ms):
        return {k: dict(ms_median=round(med(v), 5), ms_min=round(min(v), 5), ms_max=round(max(v), 5)) for k, v in ms.items()}

    res = dict(rounds=a.rounds, warmup=a.warmup, inner=a.inner, atomic_rate_guide_TBs=ATOMIC_GUIDE_TBS)
    with torch.no_grad():
        # ---- (a) chair, 800 x 800
        _, opt_fn, points_fn, n_points, _ = bench._cfg()["chair"]
        opt = opt_fn(is_train=0)
        model = bench.build_model(opt, n_points, dev, points_fn)
        d = scenes.block_rays(theta_deg=30.0, size=1)                      # the pose of configs[0]; only its camera is used
        t = lambda x: torch.from_numpy(x).to(dev)
        cam = (t(d["campos"]), t(d["camrotc2w"]), t(d["intrinsic"][0]), SIZE, SIZE, t(d["near"]), t(d["far"]))
        bg = t(d["bg_color"])
        n = int(model.neural_points.xyz.shape[0])
        rgb = torch.rand(n, 3, device=dev)
        image = torch.rand(SIZE, SIZE, 3, device=dev)

        def plain_chunks():
            for _ in point_maps._dense_chunks(model, *cam, bg, a.chunk):
                pass
        ms = rounds(dict(render_image=(lambda: eval_loop.render_image(model, *cam, bg, chunk=a.chunk), 1), render_dense_chunks=(plain_chunks, 1),
                         render_point_maps_C3=(lambda: point_maps.render_point_maps(model, rgb, *cam, bg_color=bg, chunk=a.chunk), 1),
                         render_point_maps_pick=(lambda: point_maps.render_point_maps(model, None, *cam, bg_color=bg, chunk=a.chunk), 1),
                         lift_image_C3=(lambda: point_maps.lift_image(model, image, *cam, bg_color=bg, chunk=a.chunk), 1),
                         lift_image_mass=(lambda: point_maps.lift_image(model, None, *cam, bg_color=bg, chunk=a.chunk), 1)))
        maps = point_maps.render_point_maps(model, rgb, *cam, bg_color=bg, chunk=a.chunk)
        res["chair"] = dict(view=[SIZE, SIZE], chunk=a.chunk, K=int(opt.K), SR=int(opt.SR), n_points=n, hit_rays=int(maps["hit"].sum()),
                            picked_pixels=int((maps["top_point"] >= 0).sum()), **summary(ms))
        res["chair"]["render_image_spread_ms"] = round(max(ms["render_image"]) - min(ms["render_image"]), 5)
        del model
        # ---- (b) lego, two chunks of random rays
        _, opt_fn, points_fn, n_points, _ = bench._cfg()["lego"]
        opt = opt_fn(is_train=0)
        model = bench.build_model(opt, n_points, dev, points_fn)
        n = int(model.neural_points.xyz.shape[0])
        tables = {C: torch.rand(n, C, device=dev) for C in (1, 3, 32)}
        res["lego"] = dict(rays=LEGO_RAYS, K=int(opt.K), SR=int(opt.SR), n_points=n, chunks=[])
        ok = True
        for step in (0, 1):
            inp = bench.step_inputs(step, 0, 1, LEGO_RAYS, dev)
            render = lambda: model.render_dense(inp["campos"], inp["raydir"], inp["camrotc2w"], inp["near"], inp["far"], inp["bg_color"], train=False)
            tt = render()
            bw, w, pidx, hit = tt[3].clone(), tt[5].clone(), tt[7]["sample_pidx"].clone(), tt[7]["ray_hit"].clone()
            R, SR, K = (int(x) for x in w.shape)
            hitb = hit > 0
            active = (bw != 0) & hitb[:, None]
            g = (bw[:, :, None] * w) * ((pidx >= 0) & (pidx < n)) * active[:, :, None]
            n_hit, n_active, n_entries = int(hitb.sum()), int(active.sum()), int((g != 0).sum())
            del g
            values = {C: torch.rand(R, C, device=dev) for C in (3,)}
            acc = {C: (torch.zeros(n, C, device=dev), torch.zeros(n, device=dev)) for C in (0, 3)}
            items = dict(render_dense=(render, 1))
            for C in (0, 1, 3, 32):
                items["ray_attributes_C%d" % C] = ((lambda C=C: ops.ray_attributes(tables.get(C), bw, w, pidx, hit, n_points=n)), a.inner)
            for C in (0, 3):
                items["lift_to_points_C%d" % C] = ((lambda C=C: ops.lift_to_points(values.get(C), None, bw, w, pidx, hit, n, out=acc[C])), a.inner)
            ms = rounds(items)
            row = dict(step=step, hit_rays=n_hit, samples_with_blend_weight=n_active, entries=n_entries, **summary(ms))
            row["render_dense_spread_ms"] = round(max(ms["render_dense"]) - min(ms["render_dense"]), 5)
            read = R * 4 + n_hit * SR * 4 + n_active * K * 8
            for C in (0, 1, 3, 32):
                k = "ray_attributes_C%d" % C
                row[k]["bytes"] = read + n_entries * C * 4 + R * (C + 3) * 4
                row[k]["GBs"] = round(row[k]["bytes"] / row[k]["ms_median"] / 1e6, 2)
            for C in (0, 3):
                k = "lift_to_points_C%d" % C
                row[k]["bytes"] = read + n_hit * C * 4 + n_entries * (C + 1) * 4
                row[k]["GBs"] = round(row[k]["bytes"] / row[k]["ms_median"] / 1e6, 2)
                row[k]["added_bytes"] = n_entries * (C + 1) * 4
                row[k]["added_TBs"] = round(row[k]["added_bytes"] / row[k]["ms_median"] / 1e9, 4)
            row["within"] = bool(row["ray_attributes_C3"]["ms_median"] + row["render_dense_spread_ms"] < row["render_dense"]["ms_median"])
            ok = ok and row["within"]
            res["lego"]["chunks"].append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert ok, "ray_attributes at C = 3 does not stay below the plain render of its chunk: %s" % [
        (r["ray_attributes_C3"]["ms_median"], r["render_dense_spread_ms"], r["render_dense"]["ms_median"]) for r in res["lego"]["chunks"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls of a small op inside one event pair")
    ap.add_argument("--chunk", type=int, default=160000)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_maps.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--warmup", str(a.warmup),
           "--inner", str(a.inner), "--chunk", str(a.chunk), "--out", a.out]
    rc = subprocess.call(cmd)
    if rc != 0:
        raise SystemExit("time_point_maps: the measurement ended with status %d" % rc)


if __name__ == "__main__":
    main()

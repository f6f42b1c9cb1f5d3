"""Time a render-only pass with early ray termination (NeuralPointsRayMarching.transmittance_cutoff / cutoff_stage) at the
bench's lego configuration: chunks of 160 000 rays, cutoff c in {0, 1e-3, 1e-2}, stage width B in {8, 16, 32}, on

    (a) the bench's synthetic scene as it is, and
    (b) the same scene with alpha_branch.0.bias raised until the median bg_trans of the hit rays is below 1e-3: an opaque stand-in for a
        trained scene (NOT a trained scene: the saving on real checkpoints is not measured here).

    python tools/time_render_cutoff.py [--chunks 2] [--repeats 5] [--warmup 2] [--out profiles/render_cutoff.json]

The parent process never touches the GPU: each scene is measured by a child of its own under `timeout`, one after the other, and nothing
more is started after a child that did not exit cleanly.  A child times each setting with device events around whole passes (a pass = every
chunk rendered once through model(**inputs) under no_grad, the settings applied with eval_loop.cut_setting -- the mechanism behind the
``transmittance_cutoff=`` / ``cutoff_stage=`` keywords of render_image and test_views) and reports, per setting: rays/s from the median pass,
the run-to-run spread (max - min) / median over its repeats, the share of the valid samples that were shaded, the rays that were cut, the
render's kernel launches per chunk (counted from the launch structure, the query's excluded) and the largest change of any colour channel
against c = 0.  c = 0 runs the code a model without the option runs; ``--plain`` times exactly that without touching the attributes, and
``--root DIR`` imports the package and bench.py from another checkout (built there), which is how the c = 0 row is compared with another
commit on the same machine."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFFS = (1e-3, 1e-2)
STAGES = (8, 16, 32)
RAYS = 160000


def launches_per_chunk(K, SR, B=None):
    """kernel launches of one render (without the query's): per aggregator pass the class partition (flags + 3 scan + gather per class), one
    tile kernel per class and the colour kernel; the cut render adds the stage step and its 3-kernel compaction per stage, and the totals"""
    ncls = 3 if K % 4 == 0 else 1
    agg = 5 * ncls + ncls + 1
    if B is None:
        return agg + 1
    n_stages = (SR + min(B, SR) - 1) // min(B, SR)
    return n_stages * (4 + agg) + 2


def child(a):
    sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
    import torch
    import bench
    from pointnerf_amd import eval_loop

    assert torch.cuda.is_available(), "this measurement needs an MI355X"
    dev = torch.device("cuda:0")
    _, opt_fn, points_fn, n_points, rays_fn = bench._cfg()["lego"]
    opt = opt_fn(is_train=0)
    model = bench.build_model(opt, n_points, dev, points_fn)
    inputs = [bench.step_inputs(i, 0, 1, RAYS, dev, rays_fn) for i in range(a.chunks)]
    K, SR = int(opt.K), int(opt.SR)

    def render_all(keep=False):
        outs = []
        with torch.no_grad():
            for inp in inputs:
                t = model.render_dense(inp["campos"], inp["raydir"], inp["camrotc2w"], inp["near"], inp["far"], inp["bg_color"])
                if keep:
                    outs.append((t[0].clone(), t[2].clone(), t[7]["ray_hit"] > 0, dict(model.last_stats.items())))
        return outs

    def timed():
        ms = []
        for i in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.no_grad():
                for inp in inputs:
                    model(**inp)
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        return dict(pass_ms_median=round(med, 3), pass_ms_min=round(ms[0], 3), pass_ms_max=round(ms[-1], 3), spread=round((ms[-1] - ms[0]) / med, 4),
                    rays_per_s=round(len(inputs) * RAYS / (med * 1e-3)))

    res = {"scene": a.scene, "rays_per_chunk": RAYS, "chunks": len(inputs), "repeats": a.repeats, "K": K, "SR": SR}
    shift = 0.0
    if a.scene == "b":
        # raise the density bias until the scene is opaque: median transmittance behind the hit rays below 1e-3
        bias = model.aggregator.alpha_branch[0].bias
        for shift in (0.0, 25.0, 50.0, 100.0, 200.0, 400.0, 800.0, 1600.0):
            with torch.no_grad():
                bias.add_(shift - float(res.get("bias_shift", 0.0)))
            res["bias_shift"] = shift
            full = render_all(keep=True)
            med = float(torch.cat([bt[hit] for _, bt, hit, _ in full]).median())
            if med < 1e-3:
                break
        res["median_bg_trans_of_hit_rays"] = med
        assert med < 1e-3, "the scene did not become opaque"
    base = render_all(keep=True)
    res["valid_samples"] = sum(s["n_valid_samples"] for *_, s in base)
    res["hit_rays"] = sum(s["rays_hit"] for *_, s in base)
    if a.scene != "b":
        res["median_bg_trans_of_hit_rays"] = float(torch.cat([bt[hit] for _, bt, hit, _ in base]).median())
    rows = []
    if a.plain:
        rows.append(dict(c=0.0, B=None, route="plain (the attributes are never touched)", launches_per_chunk=launches_per_chunk(K, SR), **timed()))
    else:
        with eval_loop.cut_setting(model, 0.0, 16):
            rows.append(dict(c=0.0, B=None, route="uncut", launches_per_chunk=launches_per_chunk(K, SR), share_shaded=1.0, rays_cut=0, max_colour_change=0.0, **timed()))
        for c in CUTOFFS:
            for B in STAGES:
                with eval_loop.cut_setting(model, c, B):
                    t = timed()
                    outs = render_all(keep=True)
                change = max(float((o[0] - b[0]).abs().max()) for o, b in zip(outs, base))
                shaded = sum(s["n_shaded_samples"] for *_, s in outs)
                rows.append(dict(c=c, B=B, route="cut", launches_per_chunk=launches_per_chunk(K, SR, B), share_shaded=round(shaded / max(res["valid_samples"], 1), 4),
                                 rays_cut=sum(s["rays_cut"] for *_, s in outs), max_colour_change=change, **t))
                assert change <= 1.002 * c + 1e-4, (c, B, change)
        with eval_loop.cut_setting(model, 0.0, 16):                   # the uncut route again, last: the drift of the machine over the run
            rows.append(dict(c=0.0, B=None, route="uncut (repeated at the end)", launches_per_chunk=launches_per_chunk(K, SR), **timed()))
    res["rows"] = rows
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("a", "b"), default=None, help="measure ONE scene in this process (what the parent starts)")
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain", action="store_true", help="time only the render of a model whose attributes are never touched")
    ap.add_argument("--root", default=None, help="import pointnerf_amd and bench.py from this checkout instead of this file's")
    ap.add_argument("--timeout", type=int, default=420, help="seconds each child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_cutoff.json"))
    a = ap.parse_args()
    if a.scene is not None:
        return child(a)
    merged = {}
    for scene in ("a", "b"):
        part = a.out + "." + scene
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--scene", scene, "--chunks", str(a.chunks),
               "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--out", part] + (["--plain"] if a.plain else []) + (["--root", a.root] if a.root else [])
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit("time_render_cutoff: scene %s ended with status %d; nothing more is started" % (scene, rc))
        with open(part) as f:
            merged["scene_" + scene] = json.load(f)
        os.remove(part)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

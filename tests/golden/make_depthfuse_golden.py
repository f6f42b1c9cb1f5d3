#!/usr/bin/env python3
"""Writes tests/golden/refdepthfuse.npz: what the reference's own depth filter and visual hull compute, on CPU float32, for the cases of
tests/depthfuse_case.py (run where the reference tree lies; the suite only reads the committed .npz).

    python tests/golden/make_depthfuse_golden.py [reference root, default /root/reference]

The reference's lines are exec'ed from its source text, so that cv2 / tqdm need not import:
  models/mvs/filter_utils.py:146-297   range_mask_torch, reproject_with_depth_gpu, check_geometric_consistency_gpu, filter_by_masks_gpu,
                                       reassign_conf
  models/mvs/mvs_utils.py:573-607      alpha_masking
Stored, numeric arrays only: the inputs; per input set the dense geo_mask_sum / depth_est_averaged (captured by wrapping the exec'ed
reproject / check functions and accumulating their results with the statements of :253-259); the three returned lists of every list case;
the hull masks.

It also MEASURES the margins that tests/depthfuse_case.py records (the reference's own fp32 deviation from the float64 restatement there),
asserts that the constants in that file are the measured ones, that the reference obeys the rule the kernel is held to (decided => equal to
float64) and that at most 1 % of any case's pairs are undecided.  If a case breaks either, change its seed or noise -- not the cap."""
import os
import sys
import textwrap

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import depthfuse_case as DC          # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


def ref_lines(path, first, last, must_start):
    src = open(os.path.join(REF, path)).read().split("\n")
    block = textwrap.dedent("\n".join(src[first - 1:last]))
    assert block.lstrip().startswith(must_start), (path, first, block[:120])
    return block


class TorchRecorder:
    """`torch` for the exec'ed alpha_masking: records the argument of floor (the projected pixel), everything else is torch's"""
    def __init__(self):
        self.floored = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def floor(self, x):
        self.floored.append(x.clone())
        return torch.floor(x)


def run_filter(env, inp, opt):
    """filter_by_masks_gpu on one input set; -> lists, dense geo / avg, per-pair fp32 dist / rel [V,V,H,W]"""
    V, H, W = inp["depth"].shape
    rec = {"repro": [], "check": []}
    orig_repro, orig_check = env["_orig_repro"], env["_orig_check"]

    def repro(*a):
        out = orig_repro(*a)
        rec["repro"].append([t.clone() for t in out[:3]])                 # depth_reprojected (before :216 zeroes it), x, y
        return out

    def check(*a):
        out = orig_check(*a)
        rec["check"].append((out[0].clone(), out[2].clone()))             # geo_mask, depth_reprojected (zeroed where it failed)
        return out

    env["reproject_with_depth_gpu"], env["check_geometric_consistency_gpu"] = repro, check
    lists = env["filter_by_masks_gpu"](*DC.list_args(inp), opt)
    depth = torch.from_numpy(inp["depth"])
    y_ref, x_ref = torch.meshgrid(torch.arange(0, H), torch.arange(0, W), indexing="ij")
    dist = np.full((V, V, H, W), np.nan, np.float32)
    rel = np.full((V, V, H, W), np.nan, np.float32)
    geo = np.zeros((V, H, W), np.int32)
    avg = np.zeros((V, H, W), np.float32)
    k = 0
    for r in range(V):
        sum_srcview_depth_ests, geo_mask_sum = 0, 0
        for s in range(V):
            if s == r:
                continue
            d_rep, x_rep, y_rep = rec["repro"][k]
            geo_mask, d_zeroed = rec["check"][k]
            k += 1
            dist[r, s] = torch.sqrt((x_rep - x_ref) ** 2 + (y_rep - y_ref) ** 2).numpy()          # :209
            rel[r, s] = (torch.abs(d_rep - depth[r]) / depth[r]).numpy()                          # :212-213
            geo_mask_sum += geo_mask.to(torch.int32)                                              # :256
            sum_srcview_depth_ests += d_zeroed                                                    # :257
        if V > 1:
            geo[r] = geo_mask_sum.numpy()
        avg[r] = ((sum_srcview_depth_ests + depth[r]) / (geo_mask_sum + 1)).numpy()               # :259
    assert k == len(rec["repro"]) == len(rec["check"]) == V * (V - 1)
    return lists, geo, avg, dist, rel


def main():
    env = dict(torch=torch, F=F, np=np, tqdm=lambda x: x)
    exec(ref_lines("models/mvs/filter_utils.py", 146, 297, "def range_mask_torch(xyz_world, xyz_ref, confidence_filtered, opt):"), env)
    env["_orig_repro"], env["_orig_check"] = env["reproject_with_depth_gpu"], env["check_geometric_consistency_gpu"]
    henv = dict(torch=TorchRecorder(), print=lambda *a, **k: None)
    exec(ref_lines("models/mvs/mvs_utils.py", 573, 607, "def alpha_masking(points, alphas, intrinsics, c2ws, w2cs, near_far, opt=None):"), henv)

    fix, meas = {}, dict(dist=0.0, rel=0.0, avg=0.0, px=0.0, z=0.0)
    per_case = {}
    # ---- pass 1: run the reference, measure its deviation from float64
    for name in DC.VARIANTS:
        key = DC.VARIANTS[name][0]
        inp = DC.make_inputs(key)
        lists, geo, avg, dist32, rel32 = run_filter(env, inp, DC.make_opt(name))
        per_case[name] = (inp, lists, geo, avg, dist32, rel32)
        d64, r64, _ = DC.pairs64(inp["depth"], inp["K"], inp["E"])
        with np.errstate(all="ignore"):
            near = (d64 < 2) & (r64 < 0.02)                      # where a deviation can change a verdict (depthfuse_case.py's header)
            if near.any():
                meas["dist"] = max(meas["dist"], float(np.abs(dist32.astype(np.float64) - d64)[near].max()))
                meas["rel"] = max(meas["rel"], float(np.abs(rel32.astype(np.float64) - r64)[near].max()))
    tau_d, tau_r = 4 * meas["dist"], 4 * meas["rel"]
    # ---- pass 2: the rule on the reference itself, the cap, the depth bar
    e2e_ok = []
    for name, (inp, lists, geo, avg, dist32, rel32) in per_case.items():
        key, cnsst = DC.VARIANTS[name][0], DC.VARIANTS[name][1]
        v64 = DC.verdicts64(inp["depth"], inp["K"], inp["E"], tau_d, tau_r)
        V = inp["depth"].shape[0]
        with np.errstate(all="ignore"):
            pass32 = (dist32 < 1) & (rel32 < 0.01)
        wrong = (pass32 != v64["passing"]) & v64["decided"] & ~np.eye(V, dtype=bool)[:, :, None, None]
        assert not wrong.any(), "%s: the reference's fp32 verdict differs from float64 on %d decided pairs" % (name, wrong.sum())
        assert v64["undecided_fraction"] <= DC.UNDECIDED_CAP, (name, v64["undecided_fraction"])
        ok = v64["all_decided"]
        assert np.array_equal(geo[ok], v64["geo"][ok])
        with np.errstate(all="ignore"):
            err = np.abs(avg.astype(np.float64) - v64["avg"])[ok]
        meas["avg"] = max(meas["avg"], float(err[np.isfinite(err)].max()))
        # both sides of both tests occur
        with np.errstate(all="ignore"):
            d64, r64 = v64["dist"], v64["rel"]
            if key == "v5":                      # the depth test decides alone, both tests fail together, pairs pass
                assert ((d64 < 1) & (r64 >= 0.01)).any() and ((d64 >= 1) & (r64 >= 0.01)).any() and v64["passing"].any()
            if key == "v6":                      # the pixel test decides alone
                assert ((d64 >= 1) & (r64 < 0.01)).any()
        # a case for the end-to-end comparison: every pixel the masks leave has all its pairs decided or cannot change sides, and no kept
        # pixel averages over an undecided pair (its depth_avg would legitimately differ by a whole term)
        und = (~v64["decided"]).sum(1)
        lo = (v64["passing"] & v64["decided"]).sum(1)
        live = (inp["conf"] > DC.CONF_THRESH) & inp["pmask"]
        flips = live & ((lo >= cnsst) != (lo + und >= cnsst))
        kept_und = live & (lo + und >= cnsst) & (und > 0)
        print("%-10s undecided %.4f %%  boundary pixels %d  kept pixels with an undecided pair %d  kept %d" %
              (name, 100 * v64["undecided_fraction"], flips.sum(), kept_und.sum(), sum(len(x) for x in lists[0])))
        if V > 1 and name in DC.LIST_CASES and not flips.any() and not kept_und.any():
            e2e_ok.append(name)
        # ---- store
        if key + "_depth" not in fix:
            fix[key + "_depth"], fix[key + "_K"], fix[key + "_E"] = inp["depth"], inp["K"], inp["E"]
            if not (inp["conf"] == 1).all():
                fix[key + "_conf"], fix[key + "_pmask"] = inp["conf"], inp["pmask"].astype(np.uint8)
            fix[key + "_geo"], fix[key + "_avg"] = geo.astype(np.int8), avg
        if name in DC.LIST_CASES:
            fix[name + "_sizes"] = np.array([len(x) for x in lists[0]], np.int64)
            fix[name + "_out_xyz_cam"] = torch.cat(lists[0]).numpy()
            fix[name + "_out_xyz_world"] = torch.cat(lists[1]).numpy()
            fix[name + "_out_conf"] = torch.cat(lists[2]).numpy()
            assert 0 < len(fix[name + "_out_conf"]) < inp["depth"].size or V == 1, name
    print("cases fit for the end-to-end comparison:", e2e_ok)
    assert DC.E2E_CASE in e2e_ok, "pick one of %s as depthfuse_case.E2E_CASE" % e2e_ok

    # ---- the hull
    h = DC.make_hull_inputs()
    pts, alphas, K, E = h["points"], h["alphas"], h["K"], h["E"]
    V, H, W = alphas.shape
    fix.update(hull_points=pts, hull_alphas=alphas, hull_K=K, hull_E=E)
    tp = torch.from_numpy(pts)
    runs = []
    for i, (with_nf, inall) in enumerate(DC.HULL_COMBOS):
        nf = DC.HULL_NEAR_FAR if with_nf else None
        import types
        opt = types.SimpleNamespace(alpha_range=0, inall_img=inall)
        henv["torch"].floored.clear()
        mask = henv["alpha_masking"](tp, [alphas[v][None] for v in range(V)], [K[v] for v in range(V)], [np.linalg.inv(E[v]) for v in range(V)],
                                     [E[v] for v in range(V)], nf, opt=opt)
        fix["hull_mask_%d" % i] = mask.numpy().astype(np.uint8)
        px32 = np.stack([f.numpy() for f in henv["torch"].floored])                                   # [V,N,2]
        w_xyz1 = torch.cat([tp, torch.ones_like(tp[..., :1])], dim=-1)
        z32 = np.stack([(w_xyz1 @ torch.from_numpy(E[v]).t())[..., 2].numpy() for v in range(V)])     # :581, the same statement
        want, px64, z64 = DC.hull64(pts, alphas, K, E, nf, inall == 0)
        with np.errstate(all="ignore"):
            near = (px64[..., 0] > -1) & (px64[..., 0] < W + 1) & (px64[..., 1] > -1) & (px64[..., 1] < H + 1)
            meas["px"] = max(meas["px"], float(np.abs(px32.astype(np.float64) - px64)[near].max()))
            meas["z"] = max(meas["z"], float(np.abs(z32.astype(np.float64) - z64).max()))
        runs.append((mask.numpy(), want, px64, z64, nf))
    for mask, want, px64, z64, nf in runs:
        ok = DC.hull_decided(px64, z64, H, W, nf, 4 * meas["px"], 4 * meas["z"])
        assert (~ok).mean() <= DC.UNDECIDED_CAP, (~ok).mean()
        assert np.array_equal(mask[ok], want[ok]), "the reference's hull differs from float64 on decided points"
        print("hull: kept %d of %d, undecided %d" % (want.sum(), len(want), (~ok).sum()))

    out = os.path.join(HERE, "refdepthfuse.npz")
    np.savez_compressed(out, **fix)
    print("wrote %s: %d bytes, %d arrays" % (out, os.path.getsize(out), len(fix)))
    assert os.path.getsize(out) < 1024 * 1024
    print("measured (record in tests/depthfuse_case.py):")
    print("REF_DEV_DIST, REF_DEV_REL, REF_DEV_AVG = %.3e, %.3e, %.3e" % (meas["dist"], meas["rel"], meas["avg"]))
    print("REF_DEV_PX, REF_DEV_Z = %.3e, %.3e" % (meas["px"], meas["z"]))
    rec = (DC.REF_DEV_DIST, DC.REF_DEV_REL, DC.REF_DEV_AVG, DC.REF_DEV_PX, DC.REF_DEV_Z)
    now = tuple(float("%.3e" % meas[k]) for k in ("dist", "rel", "avg", "px", "z"))
    assert rec == now, "tests/depthfuse_case.py records %s, measured %s" % (rec, now)


if __name__ == "__main__":
    main()

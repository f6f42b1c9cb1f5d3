#!/usr/bin/env python3
"""Writes tests/golden/refcloudinit.npz: what the reference's own lines of the `--load_points` route compute, on CPU float32, for the cases
of tests/cloudinit_case.py (run where the reference tree lies; the suite only reads the committed .npz).

    python tests/golden/make_cloudinit_golden.py [reference root, default /root/reference]

The reference's lines are exec'ed from its source text (none of it is stored), so that cv2 / tqdm / torch_scatter need not import:
  run/train_ft.py:39-48               nearest_view
  models/mvs/mvs_utils.py:520-534     construct_vox_points_ind
  run/train_ft.py:657-669             the occupancy merge (:658-669 with filter_res preset for the second resolution)
  run/train_ft.py:675-680             the crop to opt.ranges
  run/train_ft.py:707-710             nearest view, unique, the split into per-view lists
Stored, numeric arrays only: the inputs; the reference's camera index per nearest-view case; the merge masks; the cropped rows; the grouped
lists of the end-to-end case.

It also MEASURES REF_DEV (the largest |score32 - score64| of the reference's nearest_view over all cases; the fp32 scores are captured by
handing the exec'ed function a `torch` whose argmin records its argument), asserts that tests/cloudinit_case.py records the measured value,
that the reference obeys the rule the kernel is held to (decided => the float64 argmin, undecided => within 2 TAU of the best), that at
most 1 % of any case's points are undecided, and that E2E_CASE has no undecided point among the points that reach nearest_view.  If a case
breaks the cap, change its seed or geometry -- not the cap."""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import cloudinit_case as CC          # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


def ref_lines(path, first, last, must_start):
    src = open(os.path.join(REF, path)).read().split("\n")
    block = textwrap.dedent("\n".join(src[first - 1:last]))
    assert block.lstrip().startswith(must_start), (path, first, block[:120])
    return block


class TorchRecorder:
    """`torch` for the exec'ed nearest_view: records the argument of argmin (the [slice, M] scores), everything else is torch's"""
    def __init__(self):
        self.scores = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def argmin(self, x, *a, **k):
        self.scores.append(x.clone())
        return torch.argmin(x, *a, **k)


def main():
    rec = TorchRecorder()
    nenv = dict(torch=rec)
    exec(ref_lines("run/train_ft.py", 39, 48, "def nearest_view(campos, raydir, xyz, id_list):"), nenv)
    menv = dict(torch=torch)
    exec(ref_lines("models/mvs/mvs_utils.py", 520, 534, "def construct_vox_points_ind(xyz_val, vox_res, partition_xyz=None, space_min=None, space_max=None):"), menv)
    mvs_utils = types.SimpleNamespace(construct_vox_points_ind=menv["construct_vox_points_ind"])
    merge_100 = ref_lines("run/train_ft.py", 657, 669, "filter_res = 100")
    merge_any = ref_lines("run/train_ft.py", 658, 669, "pc_grid_id, _, pc_space_min, pc_space_max = mvs_utils.construct_vox_points_ind(points_xyz_all, filter_res)")
    crop = ref_lines("run/train_ft.py", 675, 680, "if opt.ranges[0] > -99.0:")
    split = ref_lines("run/train_ft.py", 707, 710, "cam_ind = nearest_view(campos, camdir, points_xyz_all, train_dataset.id_list)")

    def nearest(inp):
        """-> cam_ind [N] int64, fp32 scores [N,M]"""
        rec.scores.clear()
        out = nenv["nearest_view"](torch.from_numpy(inp["campos"]), torch.from_numpy(inp["camdir"]), torch.from_numpy(inp["xyz"]), None)
        M = len(inp["campos"])
        s32 = torch.cat(rec.scores).numpy() if rec.scores else np.zeros((0, M), np.float32)
        assert out.dtype == torch.int64 and tuple(out.shape) == (len(inp["xyz"]), 1) and s32.shape == (len(inp["xyz"]), M)
        return out.numpy()[:, 0], s32

    def merge(a, b, res):
        env = dict(torch=torch, mvs_utils=mvs_utils, points_xyz_all=torch.from_numpy(a), depth_xyz_all=torch.from_numpy(b), filter_res=res)
        exec(merge_100 if res == 100 else merge_any, env)
        assert env["filter_res"] == res
        return (env["depth_maskinds"] > 0).numpy(), env["depth_xyz_all"]

    def cropped(pts, ranges):
        env = dict(torch=torch, opt=types.SimpleNamespace(ranges=ranges), points_xyz_all=pts)
        exec(crop, env)
        return env["points_xyz_all"]

    fix, dev = {}, 0.0
    # ---- nearest view, pass 1: run the reference, measure its deviation from float64
    runs = {}
    for name in CC.NV_CASES:
        inp = CC.make_nv_inputs(name)
        cam, s32 = nearest(inp)
        s64 = CC.score64(inp["xyz"], inp["campos"], inp["camdir"])
        if s64.size:
            dev = max(dev, float(np.abs(s32.astype(np.float64) - s64).max()))
        runs[name] = (inp, cam, s64)
        for k in ("xyz", "campos", "camdir"):
            fix["nv_%s_%s" % (name, k)] = inp[k]
        fix["nv_%s_cam_ind" % name] = cam.astype(np.int16)
    tau = 4 * dev
    # ---- pass 2: the rule on the reference itself, the cap
    for name, (inp, cam, s64) in runs.items():
        twin = CC.NV_CASES[name][5]
        ok, und, msg = CC.obeys_rule(cam, s64, twin, tau)
        print("%-12s N %5d M %4d  %s" % (name, len(cam), s64.shape[1], msg))
        assert ok, (name, msg)
        assert und <= CC.UNDECIDED_CAP, (name, und)
        if twin is not None:
            assert np.array_equal(inp["campos"][twin[0]], inp["campos"][twin[1]]) and not (cam == twin[1]).any() and (cam == twin[0]).any()
    x30 = runs["ring24_x30"]
    d = np.linalg.norm(x30[0]["xyz"][:, None].astype(np.float64) - x30[0]["campos"][None], axis=-1) / 200
    assert d.min() > 0.3, "the distance term does not matter in the scaled case"
    assert (x30[1] != runs["ring24"][1]).any()

    # ---- merge and crop
    m = CC.make_merge_inputs()
    fix["merge_a"], fix["merge_b"] = m["a"], m["b"]
    for res in CC.MERGE_RES:
        mask, kept = merge(m["a"], m["b"], res)
        assert np.array_equal(kept.numpy(), m["b"][mask]) and 0 < mask.sum() < len(mask)
        fix["merge_mask_%d" % res] = mask.astype(np.uint8)
        same, _ = merge(m["a"], m["a"], res)
        assert not same.any()
        print("merge res %3d: kept %d of %d" % (res, mask.sum(), len(mask)))
    fix["crop_box"] = cropped(torch.from_numpy(m["b"]), CC.CROP_RANGES["box"]).numpy()
    assert 0 < len(fix["crop_box"]) < len(m["b"]) and len(cropped(torch.from_numpy(m["b"]), CC.CROP_RANGES["nothing"])) == 0

    # ---- end to end: merge at 100 -> concatenate (:672, vox_res 0) -> crop -> nearest view -> per-view lists
    e2e_ok = []
    for name in CC.E2E_CANDIDATES:
        inp = CC.make_e2e_inputs(name)
        _, kept = merge(inp["a"], inp["b"], CC.E2E_MERGE_RES)
        pts = cropped(torch.cat([torch.from_numpy(inp["a"]), kept], dim=0), CC.E2E_RANGES)
        env = dict(torch=rec, nearest_view=nenv["nearest_view"], points_xyz_all=pts, print=lambda *a, **k: None,
                   campos=torch.from_numpy(inp["campos"]), camdir=torch.from_numpy(inp["camdir"]), train_dataset=types.SimpleNamespace(id_list=None))
        exec(split, env)
        lists, ids = env["points_xyz_all"], env["unique_cam_ind"]
        s64 = CC.score64(pts.numpy(), inp["campos"], inp["camdir"])
        ok, und, msg = CC.obeys_rule(env["cam_ind"].numpy()[:, 0], s64, None, tau)
        n_und = int(round(und * len(pts)))
        print("%-6s merge kept %d of %d, crop left %d of %d, %d groups, undecided %d" %
              (name, len(kept), len(inp["b"]), len(pts), len(inp["a"]) + len(kept), len(ids), n_und))
        assert ok, (name, msg)
        if n_und == 0 and len(kept) < len(inp["b"]) and len(pts) < len(inp["a"]) + len(kept) and 1 < len(ids) < 24:
            e2e_ok.append(name)
        if name == CC.E2E_CASE:
            for k in ("a", "b", "campos", "camdir"):
                fix["e2e_" + k] = inp[k]
            fix["e2e_xyz"] = torch.cat(lists, dim=0).numpy()
            fix["e2e_view_ids"] = ids.numpy().astype(np.int64)
            fix["e2e_sizes"] = np.array([len(x) for x in lists], np.int64)
    print("cases fit for the end-to-end comparison:", e2e_ok)
    assert CC.E2E_CASE in e2e_ok, "pick one of %s as cloudinit_case.E2E_CASE" % e2e_ok

    out = os.path.join(HERE, "refcloudinit.npz")
    np.savez_compressed(out, **fix)
    print("wrote %s: %d bytes, %d arrays" % (out, os.path.getsize(out), len(fix)))
    assert os.path.getsize(out) < 500 * 1000
    print("measured (record in tests/cloudinit_case.py):")
    print("REF_DEV = %.3e" % dev)
    assert CC.REF_DEV == float("%.3e" % dev), "tests/cloudinit_case.py records %s, measured %.3e" % (CC.REF_DEV, dev)


if __name__ == "__main__":
    main()

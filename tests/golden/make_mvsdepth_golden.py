#!/usr/bin/env python3
"""Writes tests/golden/refmvsdepth.npz: what the reference's own lines compute, on CPU float32, for the cases of tests/mvsdepth_case.py
(run where the reference tree lies; the suite only reads the committed .npz).

    python tests/golden/make_mvsdepth_golden.py <reference root>

Nothing of the reference's text is stored.  What runs:
  models/depth_estimators/module.py           homo_warping, depth_regression (imported: the package needs torch alone)
  models/depth_estimators/mvsnet.py:110-122   the variance lines, exec'ed from the source text around homo_warping
  models/depth_estimators/mvsnet.py:130-136   depth, the padded pool, the index and the gather, exec'ed on a given probability volume
  models/depth_estimators/mvsnet.py           MVSNet(refine=False).eval() end to end
  models/mvs/mvs_points_model.py:142-182      gau_single_sampler, sample_by_gau, depth2point, exec'ed as methods of a stand-in class ("cuda"
                                              replaced by "cpu" in the text), behind the two F.interpolate lines :329-331
  models/mvs/mvs_utils.py:92-98               ndc_2_cam
  models/mvs/models.py:690-764                ConvBnReLU and FeatureNet(intermediate=True), exec'ed with a STAND-IN for inplace_abn's
                                              InPlaceABN (not installed here): nn.BatchNorm2d in eval followed by leaky_relu(0.01), its default
The `align_corners=True` cost-volume case runs homo_warping's text with that argument added to its grid_sample call.
Stored, numeric arrays (and two lists of names with their shapes): the reference's outputs per case and dev_*: per case and quantity the
reference's largest fp32 deviation from the float64 restatement of tests/mvsdepth_case.py.  The tests use four times these numbers.
Asserted while writing: the reference itself obeys the decided-index rule (decided => its index is the float64 one) with at most 1 % of a
case's pixels undecided, and the end-to-end probability volume is not flat (median over pixels of the largest probability > 0.3)."""
import os
import sys
import textwrap
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import mvsdepth_case as MC          # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
REF = sys.argv[1]
sys.path.insert(0, REF)
from models.depth_estimators import module as RMod, mvsnet as RNet          # noqa: E402


def ref_lines(path, first, last, must_start):
    src = open(os.path.join(REF, path)).read().split("\n")
    block = textwrap.dedent("\n".join(src[first - 1:last]))
    assert block.lstrip().startswith(must_start), (path, first, block[:120])
    return block


def as_method_class(name, text, env):
    exec("class %s:\n" % name + "\n".join("    " + ln for ln in text.split("\n")), env)
    return env[name]


def main():
    out = {}
    t = torch.from_numpy

    # ---- 1. cost volume
    warp_src = ref_lines("models/depth_estimators/module.py", 36, 70, "def homo_warping(src_fea, proj, depth_values):")
    env_ac = dict(torch=torch, F=F)
    exec(warp_src.replace("padding_mode='zeros')", "padding_mode='zeros', align_corners=True)"), env_ac)
    assert "align_corners=True" in warp_src.replace("padding_mode='zeros')", "padding_mode='zeros', align_corners=True)")
    variance_src = ref_lines("models/depth_estimators/mvsnet.py", 110, 122, "volume_sum = 0")
    for name in MC.CV_CASES:
        feats, proj, dv, ac = MC.cv_inputs(name)
        B, V = proj.shape[:2]
        env = dict(homo_warping=env_ac["homo_warping"] if ac else RMod.homo_warping, num_views=V, self=types.SimpleNamespace(training=False),
                   features=[t(feats[v])[None].expand(B, -1, -1, -1).contiguous() for v in range(V)], proj_matrices=t(proj), depth_values=t(dv))
        with torch.no_grad():
            exec(variance_src, env)
        ref = env["volume_variance"].numpy()
        want, wild = MC.cost_volume64(feats, proj, dv, ac)
        tame = ~np.broadcast_to(wild[:, None], ref.shape)
        dev = np.abs(ref.astype(np.float64) - want)[tame].max() / float((feats.astype(np.float64) ** 2).max())
        print("cv", name, "reference deviation %.3e, wild %d" % (dev, wild.sum()))
        out["cv_%s_var" % name] = np.where(tame, ref, 0.0).astype(np.float32)          # (what the reference holds on wild voxels is undefined)
        out["dev_cv_" + name] = np.float64(dev)

    # ---- 2. depth regression
    tail_src = ref_lines("models/depth_estimators/mvsnet.py", 130, 136, "depth = depth_regression(prob_volume, depth_values=depth_values)")

    def ref_tail(cost_reg, depth_values):
        env = dict(torch=torch, F=F, depth_regression=RMod.depth_regression, prob_volume=F.softmax(cost_reg, dim=1), depth_values=depth_values,
                   num_depth=depth_values.shape[1])
        with torch.no_grad():
            exec(tail_src, env)
            fi = RMod.depth_regression(env["prob_volume"], depth_values=torch.arange(env["num_depth"], dtype=torch.float))
        return env["depth"].numpy(), env["photometric_confidence"].numpy(), env["prob_volume"].numpy(), fi.numpy(), env["depth_index"].numpy()

    def measure_tail(tag, logits, dv, ref):
        depth, conf, prob, fi32, index = ref
        d64, fi64, c64, p64 = MC.regress64(logits, dv)
        tau = 4 * np.abs(fi32 - fi64).max()
        ok = MC.decided(fi64, tau)
        und = 1 - ok.mean()
        assert und <= MC.UNDECIDED_CAP, (tag, und)
        assert np.array_equal(index[ok], np.trunc(fi64[ok]).astype(np.int64)), "the reference breaks the decided-index rule: " + tag
        out["dev_%s_depth" % tag] = np.float64(np.abs(depth - d64).max())
        out["dev_%s_idx" % tag] = np.float64(np.abs(fi32 - fi64).max())
        out["dev_%s_conf" % tag] = np.float64(np.abs(conf - c64)[ok].max())
        out["dev_%s_prob" % tag] = np.float64(np.abs(prob - p64).max())
        near3, near4 = (np.abs(fi64 - np.round(fi64)) < 1e-3).mean(), (np.abs(fi64 - np.round(fi64)) < 1e-4).mean()
        print(tag, "deviations depth %.3e idx %.3e conf %.3e prob %.3e; undecided %.4f %%; within 1e-3 / 1e-4 of an integer: %.3f %% / %.3f %%"
              % (out["dev_%s_depth" % tag], out["dev_%s_idx" % tag], out["dev_%s_conf" % tag], out["dev_%s_prob" % tag], 100 * und, 100 * near3, 100 * near4))

    for name in MC.RG_CASES:
        logits, dv = MC.rg_inputs(name)
        ref = ref_tail(t(logits), t(dv))
        measure_tail("rg_" + name, logits, dv, ref)
        out["rg_%s_depth" % name], out["rg_%s_conf" % name] = ref[0], ref[1]

    # ---- 3. depth to points
    cpu_text = lambda s: s.replace('"cuda"', '"cpu"')
    senv = dict(torch=torch)
    exec(ref_lines("models/mvs/mvs_utils.py", 92, 98, "def ndc_2_cam(ndc_xyz, near_far, intrinsic, W, H):"), senv)
    Sampler = as_method_class("Sampler", cpu_text(ref_lines("models/mvs/mvs_points_model.py", 142, 182, "def gau_single_sampler(self, volume_prob")), senv)
    for name in MC.DP_CASES:
        depth, conf, K, size = MC.dp_inputs(name)
        args = types.SimpleNamespace(num_each_depth=1, manual_std_depth=0.0)
        depths_h, pc = t(depth)[None, None], t(conf)[None, None]
        bcam = torch.nn.functional.interpolate(depths_h, size=list(size), mode="nearest")                       # :329
        pc = torch.nn.functional.interpolate(pc, size=list(size), mode="nearest")                               # :331
        std = torch.ones_like(bcam) * args.manual_std_depth                                                     # :333
        torch.manual_seed(0)
        _, cam_xyz, hdwd, mask = Sampler().gau_single_sampler(None, args, t(K)[None], torch.tensor(MC.DP_NEAR_FAR, dtype=torch.float32),
                                                              cam_expected_depth=bcam, ndc_std_depth=std)
        assert tuple(cam_xyz.shape) == (1, 1, 1) + tuple(size) + (3,) and tuple(hdwd) == tuple(size)
        want, cf64, m64 = MC.points64(depth, conf, K, size)
        assert np.array_equal(pc[0, 0].numpy(), cf64) and np.array_equal(mask[0, 0].numpy(), m64), "restated index or mask differs: " + name
        out["dp_%s_conf" % name], out["dp_%s_mask" % name] = pc[0, 0].numpy(), mask[0, 0].numpy().astype(np.uint8)
        out["dp_%s_xyz" % name] = cam_xyz[0, 0, 0].numpy()
        out["dev_dp_" + name] = np.float64(np.abs(cam_xyz[0, 0, 0].numpy().astype(np.float64) - want).max())
        print("dp", name, "reference deviation %.3e" % out["dev_dp_" + name])

    # ---- 4. end to end
    from pointnerf_amd.depth_estimators import MVSNet, PyramidFeatureNet
    imgs, proj, dv = MC.e2e_inputs()
    ref_net = MC.fill_weights(RNet.MVSNet(refine=False), MC.E2E["wseed"]).eval()
    with torch.no_grad():
        depth, conf, feats, prob = ref_net(t(imgs), t(proj), t(dv))
        _, prob2, cost = ref_net(t(imgs), t(proj), t(dv), prob_only=True)
        fi32 = RMod.depth_regression(prob, depth_values=torch.arange(dv.shape[1], dtype=torch.float)).numpy()
    assert torch.equal(prob, prob2)
    peak = float(np.median(prob.numpy().max(1)))
    print("e2e: median over pixels of the largest probability %.3f" % peak)
    assert peak > 0.3, "flat probability volume: change fill_weights"
    own = MC.fill_weights(MVSNet(), MC.E2E["wseed"])
    assert list(own.state_dict()) == list(ref_net.state_dict()), "state_dict keys differ from the reference's"
    d64, fi64, c64, p64, _ = MC.mvsnet64(own, imgs, proj, dv)
    tau = 4 * np.abs(fi32 - fi64).max()
    ok = MC.decided(fi64, tau)
    assert 1 - ok.mean() <= MC.UNDECIDED_CAP, 1 - ok.mean()
    assert np.array_equal(np.trunc(fi32)[ok], np.trunc(fi64)[ok])
    out["dev_e2e_depth"] = np.float64(np.abs(depth.numpy() - d64).max())
    out["dev_e2e_idx"] = np.float64(np.abs(fi32 - fi64).max())
    out["dev_e2e_conf"] = np.float64(np.abs(conf.numpy() - c64)[ok].max())
    out["dev_e2e_prob"] = np.float64(np.abs(prob.numpy() - p64).max())
    print("e2e deviations depth %.3e idx %.3e conf %.3e prob %.3e, undecided %.3f %%"
          % (out["dev_e2e_depth"], out["dev_e2e_idx"], out["dev_e2e_conf"], out["dev_e2e_prob"], 100 * (1 - ok.mean())))
    out["e2e_depth"], out["e2e_conf"], out["e2e_prob"] = depth.numpy(), conf.numpy(), prob.numpy()
    sd = ref_net.state_dict()
    out["mvsnet_keys"] = np.array(list(sd))
    out["mvsnet_shapes"] = np.array([list(v.shape) + [-1] * (5 - v.dim()) for v in sd.values()], np.int64)

    # ---- the pyramid, with the stand-in norm
    class InPlaceABN(nn.BatchNorm2d):
        """STAND-IN for inplace_abn.InPlaceABN in inference form: batch norm, then its default activation leaky_relu(0.01)"""
        def forward(self, x):
            return F.leaky_relu(super().forward(x), 0.01)

    penv = dict(torch=torch, nn=nn, F=F, InPlaceABN=InPlaceABN)
    exec(ref_lines("models/mvs/models.py", 690, 701, "class ConvBnReLU(nn.Module):"), penv)
    exec(ref_lines("models/mvs/models.py", 717, 764, "class FeatureNet(nn.Module):"), penv)
    ref_pyr = MC.fill_weights(penv["FeatureNet"](intermediate=True), MC.PYR["wseed"]).eval()
    own_pyr = MC.fill_weights(PyramidFeatureNet(), MC.PYR["wseed"])
    keys = [k for k in ref_pyr.state_dict() if not k.endswith("num_batches_tracked")]
    assert keys == list(own_pyr.state_dict())
    pim = MC.pyr_inputs()
    with torch.no_grad():
        levels = ref_pyr(t(pim))
    want = MC.pyramid64(own_pyr, pim)
    assert len(levels) == 4 and torch.equal(levels[0], t(pim).reshape(levels[0].shape))
    out["dev_pyr"] = np.float64(max(np.abs(l.numpy() - w).max() / np.abs(w).max() for l, w in zip(levels[1:], want[1:])))
    print("pyramid deviation %.3e" % out["dev_pyr"])
    for i in (1, 2, 3):
        out["pyr_level%d" % i] = levels[i].numpy()
    out["pyr_keys"] = np.array(keys)
    out["pyr_shapes"] = np.array([list(ref_pyr.state_dict()[k].shape) + [-1] * (4 - ref_pyr.state_dict()[k].dim()) for k in keys], np.int64)

    path = os.path.join(HERE, "refmvsdepth.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()

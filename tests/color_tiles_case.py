"""Seeded cases of tests/cases.py with the number of VALID samples forced to a given count: the colour MLP kernels walk the valid list in
64-sample tiles, one workgroup striding over them, so the counts that matter are the tile-loop edges (a single sample, one short of / exactly /
one past a tile, a partial third tile, one sample past a full round of the grid).  The rays of a case are independent, so the count is forced
by CHOOSING RAYS: a larger block of the case's camera is queried once on the host oracle, and a subset of its rays whose valid-sample counts add
up to exactly the wanted number becomes the case's ray set.  The oracle and the kernels then see the same, ordinary inputs."""
import numpy as np
import torch

from cases import CASES, build_case
from pointnerf_amd import scenes
from oracle import pyref

TILE = 64
PER_RAY = ("raydir", "gt_image", "pixel_idx")


def edge_counts(workgroups):
    """the tile-loop edges for a grid of `workgroups` colour workgroups"""
    return [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TILE * workgroups + 1]


def _subset(counts, want):
    """indices of rays (in ray order) whose counts sum to `want` exactly: a greedy prefix, then an exact subset-sum over the rays behind it"""
    order = [i for i in range(len(counts)) if counts[i] > 0]
    take, total, k = [], 0, 0
    slack = 4 * int(max(counts)) if len(order) else 0
    while k < len(order) and total + counts[order[k]] <= want - slack:
        take.append(order[k]); total += counts[order[k]]; k += 1
    rest, need = order[k:], want - total
    reach = {0: []}                                   # sum -> rays
    for i in rest:
        for s, rays in list(reach.items()):
            t = s + counts[i]
            if t <= need and t not in reach:
                reach[t] = rays + [i]
        if need in reach:
            break
    assert need in reach, "no ray subset gives %d valid samples (block too small: %d available)" % (want, int(np.sum(counts)))
    return sorted(take + reach[need])


_blocks = {}


def forced_case(name, want, size):
    """case `name` of tests/cases.py with its ray block replaced by rays of the size x size block of the same camera whose valid samples number
    exactly `want`"""
    opt, xyz, attrs, _, mlp = build_case(name)
    seed = CASES[name][3]
    key = (name, size)
    if key not in _blocks:
        big = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0 + 40 * seed, x0=400 - size // 2, y0=400 - size // 2, size=size))
        q = pyref.query(opt, xyz, big, nthreads=8)
        valid = (q["sample_pidx"][0] >= 0).any(-1).sum(-1).numpy()            # per hit ray
        counts = np.zeros(big["raydir"].shape[1], np.int64)
        counts[q["ray_mask"][0].numpy() > 0] = valid
        _blocks[key] = (big, counts)
    big, counts = _blocks[key]
    reps = -(-want // max(int(counts.sum()), 1))      # more samples than the block has: its rays again (rays are independent, repeats are ordinary input)
    idx = torch.as_tensor(_subset(np.tile(counts, reps), want), dtype=torch.long) % len(counts)
    inp = {k: (v[:, idx].contiguous() if k in PER_RAY else v) for k, v in big.items()}
    return opt, xyz, attrs, inp, mlp


# formed by k_color_backward itself (its running sums): the colour branch's biases and the 3 x 128 output layer
COLOUR_KERNEL_TENSORS = ("color_branch.0.bias", "color_branch.2.bias", "color_branch.4.bias", "color_branch.6.bias", "color_branch.6.weight")


# One valid sample, one f16 plane per operand: an element of dW is the sum over the sample's few rows of products that each carry the two
# operands' roundings (<= 2^-11 each, csrc/backward.hip k_wgrad_f16), so its error is up to 2^-10 of the terms' magnitudes on top of the 5e-4 the
# bar already allows for both sides' fp32 arithmetic; the bar's 5e-4 alone rests on many rows averaging those roundings.
ONE_SAMPLE_ONE_PLANE_BAR = 5e-4 + 2.0 ** -10


def library_count(case):
    """the number of valid samples the library's own query finds for the case (gpu_util.DEV: the device, or the emulator's host)"""
    import gpu_util
    from pointnerf_amd.point_query import lighting_fast_querier
    opt, xyz, attrs, inp, mlp = case
    dev = torch.device(gpu_util.DEV)
    raydir = inp["raydir"][0].to(dev).contiguous()
    dense = lighting_fast_querier(dev, opt).query_dense(xyz.to(dev).contiguous()[None], xyz.shape[0], float(inp["near"].min()), float(inp["far"].max()),
                                                        raydir[None], inp["campos"].to(dev))
    return int(dense["counters"][0].item())


def check_backward(case, n):
    """Gradients of the case (n valid samples) against the oracle at the bars of tests/test_gpu_backward.py (_check), every MLP tensor and every
    per-point tensor, in the default arithmetic (one f16 plane per operand of the weight-gradient GEMMs) and in the two-plane mode.
    One exemption, n == 1 with one plane: the weight tensors that come out of the one-plane GEMMs are held to ONE_SAMPLE_ONE_PLANE_BAR instead
    (measured on the emulator: block1.0.weight 5.18e-4 of its max); the tensors k_color_backward forms itself keep the bar."""
    import test_gpu_backward as TB
    from pointnerf_amd import ops
    gm_o, gp_o, probe = TB._oracle_grads(*case)
    for planes in (1, 2):
        old = ops.set_wgrad_planes(planes)
        try:
            gm, gp, _, _ = TB._hip_grads(*case, probe)
        finally:
            ops.set_wgrad_planes(old)
        for k in gm_o:
            if n == 1 and planes == 1 and k not in COLOUR_KERNEL_TENSORS:
                scale = max(float(gm_o[k].abs().max()), 1e-8)
                err = float((gm[k] - gm_o[k]).abs().max())
                print("%-28s max|grad| %.3e  err %.3e  rel %.2e  (one sample, one plane)" % (k, scale, err, err / scale))
                assert err <= ONE_SAMPLE_ONE_PLANE_BAR * scale, (k, err, scale)
            else:
                TB._check(k, gm[k], gm_o[k])
        for k in gp_o:
            TB._check(k, gp[k], gp_o[k])

"""Seeded cases of tests/cases.py with the TILE COUNT of every sample class forced, for the dynamic tile claim of k_agg_forward / k_agg_backward
(csrc/mlp_common.h): a workgroup's first tiles are static (4 in the forward, 2 in the backward), every later one is claimed from a counter,
so the counts that matter are multiples of the grid around those look-aheads -- with the grid capped at G = 1, 2, 3 workgroups
(ops.set_tile_grid) a handful of tiles reaches them all.  As in tests/color_tiles_case.py the counts are forced by CHOOSING RAYS of a larger
block of the case's camera: a sample's class follows from its last occupied neighbor slot (csrc/aggregate.hip: pn_classify), which the host
oracle's query gives per ray."""
import numpy as np
import torch

from cases import CASES, build_case
from color_tiles_case import PER_RAY
from pointnerf_amd import scenes
from oracle import pyref

NAME, SIZE = "small_k8", 120
FWD_AHEAD, BWD_AHEAD = 3, 1                 # tiles the two loops look ahead
MODES = ("small_empty", "small_both", "small_one_tile")


def tile_counts(G):
    """tile counts of the K-rows class for a grid of G workgroups: none, one, around one round of the grid, around FWD_AHEAD rounds, one past
    four rounds -- and around the rounds that are static in the two loops (FWD_AHEAD + 1 = 4 in the forward, BWD_AHEAD + 1 = 2 in the backward)"""
    T = {0, 1, G - 1, G, G + 1, FWD_AHEAD * G - 1, FWD_AHEAD * G, FWD_AHEAD * G + 1, 4 * G + 1}
    T |= {2 * G - 1, 2 * G, 2 * G + 1, 4 * G - 1, 4 * G}
    return sorted(t for t in T if t >= 0)


def sample_classes(pidx, K):
    """[..., K] neighbor slots -> class of every sample: -1 invalid, 0 / 1 / 2 = K, K/2, K/4 rows (last occupied slot in the class's range)"""
    occ = pidx >= 0
    slot = torch.arange(1, K + 1).expand_as(occ)
    hv = torch.where(occ, slot, torch.zeros_like(slot)).amax(-1)
    cls = torch.full(hv.shape, -1, dtype=torch.long)
    cls[hv > 0] = 2
    cls[hv > K // 4] = 1
    cls[hv > K // 2] = 0
    return cls


_block = {}


def _rays():
    if not _block:
        opt, xyz, attrs, _, mlp = build_case(NAME)
        seed = CASES[NAME][3]
        big = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0 + 40 * seed, x0=400 - SIZE // 2, y0=400 - SIZE // 2, size=SIZE))
        q = pyref.query(opt, xyz, big, nthreads=8)
        cls = sample_classes(q["sample_pidx"][0], opt.K)              # per hit ray
        per_hit = torch.stack([(cls == c).sum(-1) for c in range(3)], -1).numpy()
        counts = np.zeros((big["raydir"].shape[1], 3), np.int64)
        counts[q["ray_mask"][0].numpy() > 0] = per_hit
        _block.update(big=big, counts=counts)
    return _block["big"], _block["counts"]


def _fill(c0, lo, hi, have):
    """rays (indices into c0, each used once) whose class-0 counts bring `have` into [lo, hi]"""
    reach = {have: []}
    for i in range(len(c0)):
        for s, rays in list(reach.items()):
            t = s + int(c0[i])
            if t <= hi and t not in reach:
                reach[t] = rays + [i]
        hit = [s for s in reach if lo <= s <= hi]
        if hit:
            return reach[max(hit)]
    raise AssertionError("no ray subset brings the K-rows class into [%d, %d]" % (lo, hi))


def forced_case(T, mode):
    """(case, [tiles of the three classes, valid samples]): case NAME with rays whose samples give the K-rows class exactly T tiles and the small classes what `mode` says"""
    opt, xyz, attrs, _, mlp = build_case(NAME)
    big, counts = _rays()
    K = opt.K
    ts = [64 // K, 64 // (K // 2), 64 // (K // 4)]
    pure = np.nonzero((counts[:, 0] > 0) & (counts[:, 1] == 0) & (counts[:, 2] == 0))[0]
    seeds = []
    if mode == "small_both":                # one ray with K/2-row samples, one with K/4-row samples, as few K-row samples as possible
        for c in (1, 2):
            cand = np.nonzero(counts[:, c] > 0)[0]
            seeds.append(int(cand[np.argmin(counts[cand, 0] * 1000 + counts[cand].sum(-1))]))
        if T == 0:                          # no K-row sample at all: every such ray (up to 16), so that the case is more than two samples
            none = np.nonzero((counts[:, 0] == 0) & (counts[:, 1:].sum(-1) > 0))[0]
            seeds = [int(i) for i in none[:16]]
            assert counts[seeds, 1].sum() > 0 and counts[seeds, 2].sum() > 0, "no rays without K-row samples that fill both small classes"
        seeds = sorted(set(seeds))
    elif mode == "small_one_tile":          # the K/2-rows class alone, within one tile
        cand = np.nonzero((counts[:, 1] > 0) & (counts[:, 1] <= ts[1]) & (counts[:, 2] == 0))[0]
        assert len(cand), "no ray with only a few K/2-row samples"
        seeds = [int(cand[np.argmin(counts[cand, 0] * 1000 - counts[cand, 1])])]
    have = int(counts[seeds, 0].sum()) if seeds else 0
    lo, hi = (0, 0) if T == 0 else (ts[0] * (T - 1) + 1, ts[0] * T)
    assert have <= hi, "the rays that bring the small classes already hold %d K-row samples" % have
    rest = [int(i) for i in pure if int(i) not in seeds]
    fill = [] if lo <= have <= hi else [rest[i] for i in _fill(counts[rest, 0], lo, hi, have)]
    idx = torch.as_tensor(sorted(seeds + fill), dtype=torch.long)
    tot = counts[idx.numpy()].sum(0)
    tiles = [int(-(-int(tot[c]) // ts[c])) for c in range(3)]
    assert tiles[0] == T and len(idx) > 0
    if mode == "small_empty":
        assert tiles[1] == 0 and tiles[2] == 0
    elif mode == "small_both":
        assert tiles[1] > 0 and tiles[2] > 0
    else:
        assert tiles[1] == 1 and tiles[2] == 0
    inp = {k: (v[:, idx].contiguous() if k in PER_RAY else v) for k, v in big.items()}
    return (opt, xyz, attrs, inp, mlp), tiles + [int(tot.sum())]


def cases_of(T):
    """the modes that exist for T tiles of the K-rows class (T = 0 with empty small classes is no sample at all)"""
    return [m for m in MODES if not (T == 0 and m == "small_empty")]


def library_tiles(dense, opt):
    """tiles per class of the library's own query result (dense sample_pidx / ray_hit)"""
    K = opt.K
    pidx = dense["sample_pidx"].cpu().reshape(-1, opt.SR, K)[dense["ray_hit"].cpu().reshape(-1) > 0]
    cls = sample_classes(pidx, K)
    return [int(-(-int((cls == c).sum()) // (64 // (K >> c)))) for c in range(3)]


# the weight-gradient GEMMs read the saved layout, which does not depend on who ran a tile: the same bits on every grid
DETERMINISTIC = ("block1.0.weight", "block1.0.bias", "block1.2.weight", "block1.2.bias", "block3.0.weight", "block3.0.bias",
                 "block3.2.weight", "block3.2.bias", "color_branch.0.weight", "color_branch.2.weight", "color_branch.4.weight")


FEW_SAMPLES = 24


def check_against_oracle(case, tiles):
    """forward (inference kernels) and gradients (training kernels, the default arithmetic) of the case on the grid the caller has set, against
    the oracle at the bars of tests/test_gpu_render.py and tests/test_gpu_backward.py; a skipped tile shows as poison or zeros, a tile run
    twice doubles its rows' atomic contributions.
    The 5e-4 bar of the MLP tensors holds for the one-plane weight-gradient GEMMs because many rows average the operands' f16 roundings (2^-11
    each, up to 2^-10 of a term per product; tests/color_tiles_case.py: one sample alone is 5.2e-4 of a tensor's maximum off).  In a case of
    fewer than FEW_SAMPLES valid samples the tensors those GEMMs form (DETERMINISTIC) are therefore held to that file's derived bar
    5e-4 + 2^-10 against the oracle AND must be the bits the same case gives on the default grid (they do not depend on who ran a tile);
    every other tensor keeps its bar, and the case runs once more in the two-plane mode with every tensor at the bars as they are.
    The cases below FEW_SAMPLES have 1, 2, 3, 14, 16, 20 and 22 samples; measured on the device their worst such tensor is 5.45e-4 / 4.85e-4 /
    5.22e-4 of its maximum with 1 / 2 / 3 samples (the emulator: 6.29e-4) and 1.4e-4 .. 2.2e-4 with 14 .. 22; the threshold only has to lie
    above 3 samples, 24 is three tiles of the K-rows class."""
    import test_gpu_backward as TB
    import test_gpu_render as TR
    from color_tiles_case import ONE_SAMPLE_ONE_PLANE_BAR
    from pointnerf_amd import ops
    TR._compare(*case)
    gm_o, gp_o, probe = TB._oracle_grads(*case)
    few = tiles[3] < FEW_SAMPLES
    gm, gp, _, _ = TB._hip_grads(*case, probe)
    if few:
        G = ops.set_tile_grid(0)
        try:
            gm_d, _, _, _ = TB._hip_grads(*case, probe)
        finally:
            ops.set_tile_grid(G)
    for k in gm_o:
        if few and k in DETERMINISTIC:
            scale = max(float(gm_o[k].abs().max()), 1e-8)
            err = float((gm[k] - gm_o[k]).abs().max())
            print("%-28s max|grad| %.3e  err %.3e  rel %.2e  (%d samples, one plane)" % (k, scale, err, err / scale, tiles[3]))
            assert err <= ONE_SAMPLE_ONE_PLANE_BAR * scale, (k, err, scale)
            assert torch.equal(gm[k], gm_d[k]), (k, "differs from the default grid's")
        else:
            TB._check(k, gm[k], gm_o[k])
    for k in gp_o:
        TB._check(k, gp[k], gp_o[k])
    if few:
        old = ops.set_wgrad_planes(2)
        try:
            gm2, gp2, _, _ = TB._hip_grads(*case, probe)
        finally:
            ops.set_wgrad_planes(old)
        for k in gm_o:
            TB._check(k, gm2[k], gm_o[k])
        for k in gp_o:
            TB._check(k, gp2[k], gp_o[k])
    return gm, gp, probe


def training_forward_bytes(case):
    """everything a training forward leaves: the saved area byte for byte (f rows, k-major planes, masks, row metadata, class lists, the claim
    counters) and decoded / weight / ray colour"""
    from gpu_util import hip_render
    from pointnerf_amd import ops, _lib as L
    opt = case[0]
    dense, fwd, ctx = hip_render(*case, train=True)
    need = L.lib().pnerf_agg_saved_bytes(ctx["n_valid"], opt.K)
    out = [fwd["saved"][:need].clone()] + [fwd[k].clone().view(torch.int32) for k in ("decoded", "weight", "ray_color")]
    ops.ARENA.give(fwd["saved"])
    return out, library_tiles(dense, opt), int((dense["ray_hit"] > 0).sum())


def check_grids_agree(case, tiles, grids=(1, 3, 0)):
    """the same case on grids of 1, 3 and the default number of workgroups: the training forward byte-equal, the deterministic gradients
    bit-equal, the atomically summed ones within the bars of tests/test_gpu_backward.py"""
    import test_gpu_backward as TB
    from pointnerf_amd import ops
    first = None
    for G in grids:
        old = ops.set_tile_grid(G)
        try:
            fw, lt, n_hit = training_forward_bytes(case)
            assert lt == tiles[:3], ("the case does not have the forced tile counts", lt, tiles)
            gm, gp, _, _ = TB._hip_grads(*case, torch.rand(n_hit, 3, generator=torch.Generator().manual_seed(123)))
        finally:
            ops.set_tile_grid(old)
        if first is None:
            first = (fw, gm, gp)
            continue
        for i, (a, b) in enumerate(zip(fw, first[0])):
            assert torch.equal(a, b), ("training forward differs between grids", G, i)
        for k in gm:
            if k in DETERMINISTIC:
                assert torch.equal(gm[k], first[1][k]), (k, G)
            else:
                TB._check(k, gm[k], first[1][k])
        for k in gp:
            TB._check(k, gp[k], first[2][k])


def check_backward_twice(case):
    """a forward / backward / backward sequence on ONE saved area: the backward zeroes its claim counters itself (with its scale word), so the
    second backward sees what the first saw"""
    import numpy as np
    import test_gpu_backward as TB
    from gpu_util import hip_render, DEV
    from pointnerf_amd import ops
    opt = case[0]
    dev = torch.device(DEV)
    dense, fwd, ctx = hip_render(*case, train=True)
    hit = dense["ray_hit"] > 0
    g = torch.zeros(ctx["R"], 3, device=dev)
    g[hit] = torch.rand(int(hit.sum()), 3, generator=torch.Generator().manual_seed(123)).to(dev)
    lay, _ = ops.mlp_layout()
    res = []
    for _ in range(2):
        gflat = torch.zeros_like(ctx["flat"])
        grads = {k: torch.zeros_like(v) for k, v in ctx["pts_t"].items()}
        ops.render_backward(ctx["cam"], ctx["pts"], ctx["packed"], ctx["flat"], ctx["raydir"], dense, ctx["R"], opt.SR, opt.K, ctx["n_valid"], fwd, g, gflat, grads)
        res.append(({k: gflat[o:o + int(np.prod(shp))].view(shp).cpu() for k, (o, shp) in lay.items()}, {k: v.cpu() for k, v in grads.items()}))
    ops.ARENA.give(fwd["saved"])
    (gm1, gp1), (gm2, gp2) = res
    for k in gm1:
        if k in DETERMINISTIC:
            assert torch.equal(gm1[k], gm2[k]), k
        else:
            TB._check(k, gm2[k], gm1[k])
    for k in gp1:
        TB._check(k, gp2[k], gp1[k])

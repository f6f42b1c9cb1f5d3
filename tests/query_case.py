"""Query cases beyond the cubic jittered shell (test infrastructure, shared by the reference pin tests/test_oracle_query.py, the host-emulator
twin tests/test_query_cases_emu.py and the device tests of tests/test_gpu_query.py, as mix_case.py and range_case.py serve their tests).

Three families, every one a few thousand points and 36 or 37 rays:
  A  per-axis configurations: test_gpu_query._scene with query_size / vsize / vscale / kernel_size / ranges that differ per axis, so that
     swapping two axes anywhere (dilation loop, brick addressing, the occupancy field's linear index) changes the result;
  B  P overflow: the same scenes with P = 1, and with P = 2 in fat cells -- cells hold more points than P, the first P by index are kept
     (what the reference's own kernels do in canonical serial order when every uniform number they draw is 1: the reservoir slot of a further
     point is then the cell's count, which is >= P, and nothing is replaced);
  C  lattice: points on the nodes o + i (v / 2) of the half-pitch lattice of the grid (cell corners, face centres, cell centres), some of them
     twice, and sample positions that walk lattice lines through the grid and out of it at both ends.  Samples and points sit exactly on
     cell boundaries and whole shells of candidates tie in distance: the result is decided by how (p - o) / v rounds (fp32 subtract,
     correctly rounded fp32 divide, floor), by d2 = ((xx + yy) + zz) without contraction, by `d2 < far2` being strict and by the first
     maximum winning.  No camera: the explicit raypos goes to oracle_query, ref_query and woord_query_grid_point_index.

conditions(case) asserts, on the ORACLE's result alone, that the case is what it claims to be (overflow really happens, ties and integer
quotients really occur): a case that does not meet them is a bad case, not a pass.  check(case, backend) is the bit-exact comparison."""
import functools

import numpy as np
import torch

from oracle import pyref, query as oq

MAX_O = 50000
SCENES = {"s2": (2, 3000), "s5": (5, 1500)}                      # (seed, n) of test_gpu_query._scene
_ALL = dict(query_size=[1, 3, 5], vsize=[0.004, 0.006, 0.0045], vscale=[1, 2, 3], kernel_size=[5, 3, 3], ranges=[-0.3, -0.05, -0.3, 0.02, 0.3, 0.07])
A_VARIANTS = {
    "query_size_135": dict(query_size=[1, 3, 5]), "query_size_531": dict(query_size=[5, 3, 1]),
    "vsize_a": dict(vsize=[0.004, 0.006, 0.0045]), "vsize_b": dict(vsize=[0.007, 0.003, 0.005]),
    "vscale_123": dict(vscale=[1, 2, 3]), "vscale_312": dict(vscale=[3, 1, 2]),
    "kernel_533": dict(kernel_size=[5, 3, 3]), "kernel_335": dict(kernel_size=[3, 3, 5]),      # only [0] sets the layer count, all three pad the ranges
    "ranges": dict(ranges=[-0.3, -0.05, -0.3, 0.02, 0.3, 0.07]),
    "all": _ALL,
}
B_VARIANTS = {"P1": dict(P=1), "P2_fat": dict(P=2, vsize=[0.01, 0.01, 0.01])}
# name: (v, origin, vdim, K, P, SR, radius / v, overrides)
C_VARIANTS = {
    "exact": (1.0 / 128, (-0.125, -0.0625, 0.03125), (13, 10, 9), 8, 12, 16, 1.0, {}),          # every coordinate, difference and quotient is exact in fp32
    "v008": (0.008, (-0.05, -0.04, 0.012), (13, 10, 9), 8, 12, 16, 1.0, {}),
    "P3": (0.012, (-0.07, 0.013, -0.029), (11, 9, 14), 4, 3, 24, 1.5, {}),                      # P overflows
    "K1": (0.003, (0.1, 0.2, 0.3), (9, 9, 9), 1, 12, 8, 0.5, {}),
    "K16": (0.008, (-0.05, -0.04, 0.012), (13, 10, 9), 16, 20, 16, 2.0, dict(kernel_size=[5, 5, 5])),      # beyond the reference's KN = 8: oracle only
    "no_radius": (0.006, (-0.05, -0.04, 0.012), (10, 13, 6), 8, 12, 16, 0.0, dict(query_size=[1, 3, 5])),  # radius test off
}
C_RAYS, C_DEPTH = 37, 70

NAMES = (["A/%s/%s" % (v, s) for v in A_VARIANTS for s in SCENES] + ["B/%s/%s" % (v, s) for v in B_VARIANTS for s in SCENES] +
         ["C/%s" % v for v in C_VARIANTS])
OVERFLOWS_P = [n for n in NAMES if n.startswith("B/") or n == "C/P3"]
REF_NAMES = [n for n in NAMES if n != "C/K16"]                    # the reference's K-buffer holds 8


class Case:
    """what the native op takes (raypos [R,D,3] f32, xyz [N,3] f32 tensor, the grid), and for families A / B the opt and camera inputs it came from"""

    def __init__(self, name, xyz, raypos, K, SR, P, kernel_size, query_size, hp, opt=None, inp=None, varied=None):
        self.name, self.family = name, name[0]
        self.xyz, self.raypos, self.K, self.SR, self.P = xyz, raypos, K, SR, P
        self.kernel_size, self.query_size, self.hp = list(kernel_size), list(query_size), hp
        self.opt, self.inp, self.varied = opt, inp, varied

    def args(self):
        return (self.raypos, self.xyz.numpy(), self.kernel_size, self.query_size, self.SR, self.K, self.hp["scaled_vdim"], MAX_O, self.P,
                self.hp["radius"], self.hp["ranges"], self.hp["scaled_vsize"])


def _lattice(name):
    v, origin, vdim, K, P, SR, rmul, ov = C_VARIANTS[name]
    f32 = np.float32
    v, o, vdim = f32(v), np.asarray(origin, f32), np.asarray(vdim, np.int32)
    h = f32(v / f32(2))
    node = lambda i: (o + np.asarray(i, f32) * h).astype(f32)                    # fp32 throughout: points and samples share their nodes bit for bit
    rng = np.random.default_rng(sum(map(ord, name)))
    ii = np.stack(np.meshgrid(*[np.arange(2, 2 * d - 2) for d in vdim], indexing="ij"), -1).reshape(-1, 3)
    ii = ii[ii[:, 2] % 7 < 3]                                                    # slabs: empty layers between occupied ones
    ii = ii[rng.permutation(len(ii))[:len(ii) // 2]]
    ii = np.concatenate([ii, ii[:50]])                                           # exact duplicates: d2 ties between different indices
    ii = ii[rng.permutation(len(ii))]
    xyz = node(ii)
    start = rng.integers(2, 2 * int(vdim.min()) - 2, size=(C_RAYS, 3))
    axis = rng.integers(0, 3, size=C_RAYS)
    jj = np.repeat(start[:, None, :], C_DEPTH, axis=1)
    jj[np.arange(C_RAYS), :, axis] += np.arange(-3, C_DEPTH - 3)[None, :]        # the walk leaves the grid at both ends
    raypos = node(jj)
    hp = dict(ranges=np.concatenate([o, (o + vdim.astype(f32) * v).astype(f32)]), scaled_vsize=np.array([v, v, v], f32), scaled_vdim=vdim,
              radius=float(f32(rmul) * v))
    return Case("C/" + name, torch.from_numpy(xyz), raypos, K, SR, P, ov.get("kernel_size", [3, 3, 3]), ov.get("query_size", [3, 3, 3]), hp)


@functools.lru_cache(maxsize=None)
def build(name):
    fam, var = name.split("/")[:2]
    if fam == "C":
        return _lattice(var)
    import test_gpu_query as TQ
    kw = dict((A_VARIANTS if fam == "A" else B_VARIANTS)[var])
    seed, n = SCENES[name.split("/")[2]]
    opt, xyz, inp = TQ._scene(seed, n, K=8, SR=16, size=6, **kw)
    raypos, _ = pyref.ray_samples(inp["campos"], inp["raydir"], opt.z_depth_dim, float(inp["near"].min()), float(inp["far"].max()))
    return Case(name, xyz, raypos[0].numpy(), opt.K, opt.SR, opt.P, opt.kernel_size, opt.query_size, pyref.grid_hyperparameters(opt, xyz),
                opt=opt, inp=inp, varied=kw)


def _as_q(res, hp=None):
    pidx, loc, mask, info = res
    return dict(sample_pidx=torch.from_numpy(pidx)[None], sample_loc_w=torch.from_numpy(loc)[None], ray_mask=torch.from_numpy(mask)[None], info=info, hp=hp)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the oracle's result, computed once per case and shared (do not modify)"""
    c = build(name)
    return _as_q(oq.oracle_query(*c.args()), c.hp)


def reference(name):
    """the same call through the reference's own kernels (oracle/_ref; K <= 8)"""
    return _as_q(oq.ref_query(*build(name).args()))


def native(name, dev):
    """woord_query_grid_point_index on `dev` ("cpu" under emu_util.emu_backend) -> (sample_pidx, sample_loc_w, ray_mask) on the host"""
    from pointnerf_amd.point_query import woord_query_grid_point_index
    c = build(name)
    R, D = c.raypos.shape[:2]
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=dev)
    out = woord_query_grid_point_index(
        torch.zeros(1, R, 2, dtype=torch.int32, device=dev), torch.from_numpy(c.raypos)[None].to(dev), c.xyz[None].to(dev),
        torch.tensor([c.xyz.shape[0]], dtype=torch.int32, device=dev), t(c.kernel_size, torch.int32), t(c.query_size, torch.int32),
        c.SR, c.K, R, D, t(c.hp["scaled_vdim"], torch.int32), MAX_O, c.P, np.float32(c.hp["radius"]),
        t(c.hp["ranges"], torch.float32), t(c.hp["scaled_vsize"], torch.float32), 1024, 2)
    return [o.cpu() for o in out]


def check(name, backend):
    """backend: a device string (the native op there) or a callable name -> (sample_pidx, sample_loc_w, ray_mask).  The assertions of
    test_gpu_query._assert_same: shapes, dtypes, and equality of mask, indices and the bits of the positions."""
    q = oracle(name)
    pidx, loc, mask = native(name, backend) if isinstance(backend, str) else backend(name)
    assert tuple(pidx.shape) == tuple(q["sample_pidx"].shape), (name, pidx.shape, q["sample_pidx"].shape)
    assert tuple(loc.shape) == tuple(q["sample_loc_w"].shape) and tuple(mask.shape) == tuple(q["ray_mask"].shape), name
    assert pidx.dtype == torch.int32 and mask.dtype == torch.int8 and loc.dtype == torch.float32, name
    assert torch.equal(mask, q["ray_mask"]), name
    assert torch.equal(pidx, q["sample_pidx"]), (name, "samples that differ", int((pidx != q["sample_pidx"]).any(dim=-1).sum()))
    assert torch.equal(loc.view(torch.int32), q["sample_loc_w"].view(torch.int32)), name          # the bits


def check_dense(name, dev):
    """families A / B through lighting_fast_querier.query_dense: the grid's hyper-parameters from the points on `dev`, rays generated inside the
    probe kernel; hit rays against the oracle, the grid's tallies against the oracle's, overflow_P exactly where P overflows"""
    from pointnerf_amd.point_query import lighting_fast_querier
    c, q = build(name), oracle(name)
    qr = lighting_fast_querier(torch.device(dev), c.opt)
    xd = c.xyz.to(dev)
    dense = qr.query_dense(xd[None], c.xyz.shape[0], float(c.inp["near"].min()), float(c.inp["far"].max()), c.inp["raydir"].to(dev), c.inp["campos"].to(dev))
    gp = qr.last_grid.gp
    assert list(gp.vdim) == c.hp["scaled_vdim"].tolist(), (name, list(gp.vdim), c.hp["scaled_vdim"])
    assert np.array_equal(np.asarray(list(gp.ranges), np.float32), c.hp["ranges"]) and np.array_equal(np.asarray(list(gp.vsize), np.float32), c.hp["scaled_vsize"]), name
    assert np.float32(gp.radius) == np.float32(c.hp["radius"]), name
    hit = dense["ray_hit"].cpu() > 0
    assert torch.equal(hit.to(torch.int8)[None], q["ray_mask"]), name
    assert torch.equal(dense["sample_pidx"].cpu()[hit][None], q["sample_pidx"]), name
    assert torch.equal(dense["sample_loc"].cpu()[hit][None].view(torch.int32), q["sample_loc_w"].view(torch.int32)), name
    gi = qr.last_grid_info
    assert gi["n_occ"] == q["info"]["n_occ"] and gi["max_cnt"] == q["info"]["max_cnt"], (name, gi, q["info"])
    # True for all of family B; among family A for the three s2 cases whose fullest cell holds 14 or 15 points (> P = 12), the oracle says which
    assert gi["overflow_P"] is (q["info"]["ovf_P"] == 1), (name, gi, q["info"])
    assert gi["overflow_P"] or c.family != "B", (name, gi)
    assert gi["overflow_max_o"] is False, (name, gi)
    counters = dense["counters"].cpu().tolist()
    assert counters[1] == int(hit.sum()) and counters[2] == q["info"]["n_sel"] and counters[3] == q["info"]["n_neigh"], (name, counters, q["info"])


def lattice_counts(name):
    """family C, from the oracle's selected samples with numpy alone: (samples whose K-th and (K+1)-th nearest candidate within the radius tie
    in fp32 distance, samples + points whose fp32 quotient (p - o) / v is an integer on some axis).  Candidates of a sample: the points of the
    cells within (kernel_size[0] - 1) / 2 of its own (the P cap and the reference's empty voxel 0 are ignored: this counts occasions, the
    oracle decides them); d2 = ((xx + yy) + zz) in fp32."""
    c, q = build(name), oracle(name)
    f32 = np.float32
    o, v = c.hp["ranges"][:3], c.hp["scaled_vsize"]
    quot = lambda p: ((p - o).astype(f32) / v).astype(f32)
    sel = (q["sample_pidx"][0] >= 0).any(dim=-1).numpy()
    loc = q["sample_loc_w"][0].numpy()[sel]                                      # [S,3]
    xyz = c.xyz.numpy()
    qs, qp = quot(loc), quot(xyz)
    d = (xyz[None] - loc[:, None]).astype(f32)                                   # [S,N,3]
    xx, yy, zz = (d[..., 0] * d[..., 0]).astype(f32), (d[..., 1] * d[..., 1]).astype(f32), (d[..., 2] * d[..., 2]).astype(f32)
    d2 = ((xx + yy).astype(f32) + zz).astype(f32)
    reach = (c.kernel_size[0] + 1) // 2 - 1
    cand = (np.abs(np.floor(qp)[None] - np.floor(qs)[:, None]) <= reach).all(-1)
    r2 = f32(c.hp["radius"]) * f32(c.hp["radius"])
    if r2 > 0:
        cand &= d2 <= r2
    ds = np.sort(np.where(cand, d2, np.inf), axis=1)
    tied = int(((ds[:, c.K - 1] == ds[:, c.K]) & np.isfinite(ds[:, c.K])).sum())
    whole = int((qs == np.floor(qs)).any(-1).sum()) + int((qp == np.floor(qp)).any(-1).sum())
    return tied, whole


def conditions(name):
    """conditions on the CASE (the oracle's result alone), asserted before anything is compared; returns the figures"""
    c, q = build(name), oracle(name)
    info = q["info"]
    fig = dict(valid_slots=int((q["sample_pidx"] >= 0).sum()), max_cnt=info["max_cnt"], ovf_P=info["ovf_P"], vdim=c.hp["scaled_vdim"].tolist())
    assert fig["valid_slots"] > 50, (name, fig)
    assert info["ovf_max_o"] == 0, (name, info)
    if name in OVERFLOWS_P:
        assert info["ovf_P"] == 1 and info["max_cnt"] > c.P, (name, info)
    if c.family == "A":
        per_axis = [k for k, val in c.varied.items() if k != "ranges" and len(set(val)) > 1]
        assert len(set(fig["vdim"])) == 3 or per_axis, (name, fig)
    if c.family == "C":
        fig["tied_samples"], fig["integer_quotients"] = lattice_counts(name)
        assert fig["tied_samples"] >= 1 and fig["integer_quotients"] >= 1, (name, fig)
    return fig

"""CPU tests of the query oracle (oracle/query_oracle.c):
  * bit-exact against the reference's OWN kernels compiled for the host and run in canonical serial
    order (oracle/_ref) on randomised scenes incl. ragged / empty / edge cases.  Their results are
    recorded in tests/golden/ref_query.npz (PYTHONPATH=. python tests/test_oracle_query.py rewrites it): a machine without the
    reference's kernels compares against the recording, one with them compares against both and checks the recording;
  * brute-force properties that do not depend on any restatement.
"""
import os

import numpy as np
import pytest
import torch

from pointnerf_amd import config, scenes
import query_case
from oracle import pyref, query as oq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_query.npz")
_RECORD = None              # {case: result} while the recording is rewritten (__main__)
_golden = {}


def _ref(case, opt, xyz, inp):
    return _ref_of(case, lambda: pyref.query(opt, xyz, inp, impl="ref"))


def _ref_of(case, run_live):
    """the reference kernels' query result for `case`: live where oracle/_ref can be built (and then equal to the recording), else the recording"""
    if _RECORD is None and not _golden:
        with np.load(GOLDEN) as z:
            _golden.update({k: z[k] for k in z.files})
    if _RECORD is None and ("%s/sample_pidx" % case) not in _golden:
        raise AssertionError("no recording of the reference kernels for %s in %s" % (case, GOLDEN))
    rec = None if _RECORD is not None else dict(
        sample_pidx=torch.from_numpy(_golden[case + "/sample_pidx"]), sample_loc_w=torch.from_numpy(_golden[case + "/sample_loc_w"]),
        ray_mask=torch.from_numpy(_golden[case + "/ray_mask"]), info={"curand_hits": int(_golden[case + "/curand_hits"])})
    if not oq.have_ref():
        return rec
    live = run_live()
    if _RECORD is not None:
        _RECORD[case] = live
    else:
        _same(live, rec)
        assert live["info"]["curand_hits"] == rec["info"]["curand_hits"]
    return live


def _scene(seed, n, radius=0.06, size=10, **ov):
    kw = dict(K=8, SR=16, P=12, max_o=50000, ranges=[-0.3, -0.3, -0.3, 0.3, 0.3, 0.3])
    kw.update(ov)
    opt = config.lego_opt(**kw)
    xyz = torch.from_numpy(scenes.chair_points(n, seed=seed, radius=radius))
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=17.0 * seed, x0=400 - size // 2, y0=400 - size // 2, size=size))
    return opt, xyz, inp


def _same(a, b):
    assert a["sample_pidx"].shape == b["sample_pidx"].shape
    assert torch.equal(a["sample_pidx"], b["sample_pidx"])
    assert torch.equal(a["sample_loc_w"], b["sample_loc_w"])       # bit-exact floats
    assert torch.equal(a["ray_mask"], b["ray_mask"])


SCENES = [(0, 1200, 8, 16, 12), (1, 700, 4, 8, 12), (2, 3000, 8, 32, 20), (3, 300, 1, 4, 12), (4, 2000, 6, 24, 16)]


@pytest.mark.parametrize("seed,n,K,SR,P", SCENES)
def test_oracle_equals_reference_kernels(seed, n, K, SR, P):
    opt, xyz, inp = _scene(seed, n, K=K, SR=SR, P=P)
    a = pyref.query(opt, xyz, inp, impl="oracle")
    b = _ref("scene%d" % seed, opt, xyz, inp)
    assert b["info"]["curand_hits"] == 0
    assert a["info"]["ovf_P"] == 0 and a["info"]["ovf_max_o"] == 0
    _same(a, b)
    assert a["sample_pidx"].shape[1] > 0


def test_config1_chair_equals_reference_kernels():
    """BASELINE.json configs[0]: chair 64x64, 8k points, K=4, SR=32."""
    opt = config.chair_opt()
    xyz = torch.from_numpy(scenes.chair_points())
    inp = pyref.to_torch_inputs(scenes.block_rays())
    a = pyref.query(opt, xyz, inp, impl="oracle", nthreads=4)
    b = _ref("chair", opt, xyz, inp)
    _same(a, b)
    assert a["sample_pidx"].shape == (1, 3282, 32, 4)


def test_edge_cases_match_reference():
    # rays that miss everything (camera looks at an empty region)
    opt, xyz, inp = _scene(5, 500)
    inp["raydir"] = inp["raydir"] * torch.tensor([1.0, 1.0, -1.0])
    a, b = pyref.query(opt, xyz, inp, impl="oracle"), _ref("edge_miss", opt, xyz, inp)
    _same(a, b)
    assert a["sample_pidx"].shape[1] == 0 and int(a["ray_mask"].sum()) == 0
    # a single point; points outside opt.ranges; radius clipping at the grid border
    opt, xyz, inp = _scene(6, 400, ranges=[-0.05, -0.05, -0.05, 0.05, 0.05, 0.05])
    _same(pyref.query(opt, xyz, inp, impl="oracle"), _ref("edge_ranges", opt, xyz, inp))
    opt, xyz, inp = _scene(7, 1)
    _same(pyref.query(opt, xyz, inp, impl="oracle"), _ref("edge_one_point", opt, xyz, inp))
    # kernel_size 5 (two layers beyond the centre) and query_size 1 (no dilation)
    opt, xyz, inp = _scene(8, 1500, kernel_size=[5, 5, 5], query_size=[1, 1, 1])
    _same(pyref.query(opt, xyz, inp, impl="oracle"), _ref("edge_kernel5", opt, xyz, inp))
    # radius_limit_scale = 0 disables the radius test (.cu:272)
    opt, xyz, inp = _scene(9, 800, radius_limit_scale=0)
    _same(pyref.query(opt, xyz, inp, impl="oracle"), _ref("edge_no_radius", opt, xyz, inp))


@pytest.mark.parametrize("name", query_case.REF_NAMES)
def test_query_cases_equal_reference_kernels(name):
    """tests/query_case.py against the reference's own kernels: per-axis sizes (family A), P overflow (B), lattice points and samples on cell
    boundaries with tied distances (C, the K <= 8 cases: the reference's K-buffer holds 8).
    Where a cell holds more than P points the reference draws a uniform number for every further point (curand_hits > 0) and turns it into a
    slot between 0 and the cell's count so far; the point replaces a kept one when that slot is below P (query_worldcoords.cu:152-158).  The
    serial host build's shim returns u = 1, the slot is the count itself (>= P) and nothing is replaced: the first P points by index stay, in
    canonical serial order.  That is one of the outcomes the reference itself
    can produce (its seed is the wall clock), it is the rule of grid.hip (pn_cell_points: min(P, count) of the index-sorted cell), and the
    recording of it is as canonical as the others."""
    fig = query_case.conditions(name)
    a = query_case.oracle(name)
    b = _ref_of("qc/" + name, lambda: query_case.reference(name))
    print(name, fig, "curand_hits", b["info"]["curand_hits"])
    assert (b["info"]["curand_hits"] > 0) == (a["info"]["ovf_P"] == 1)
    if name in query_case.OVERFLOWS_P:
        assert b["info"]["curand_hits"] > 0
    query_case.check(name, lambda _: (b["sample_pidx"], b["sample_loc_w"], b["ray_mask"]))


def test_voxel0_quirk_is_reproduced():
    """query_worldcoords.cu:147 `voxel_idx > 0`: the cell of the first in-range point holds no points."""
    opt, xyz, inp = _scene(0, 1200)
    q = pyref.query(opt, xyz, inp)
    hp = q["hp"]
    cell = lambda p: np.floor((p - hp["ranges"][:3]) / hp["scaled_vsize"]).astype(np.int64)
    cells = cell(xyz.numpy())
    in0 = np.all(cells == cells[0], axis=1)
    hit = torch.unique(q["sample_pidx"][q["sample_pidx"] >= 0]).numpy()
    assert not np.isin(np.flatnonzero(in0), hit).any()


def test_bruteforce_properties():
    """Every returned neighbor is within the radius; when fewer than K are returned from the centre
    layer the result is a subset of the brute-force ball; -1 padding is a suffix."""
    opt, xyz, inp = _scene(2, 3000, SR=16)
    q = pyref.query(opt, xyz, inp)
    pidx, loc = q["sample_pidx"][0].numpy(), q["sample_loc_w"][0].numpy()
    r = q["hp"]["radius"]
    xn = xyz.numpy()
    rng = np.random.default_rng(0)
    rays = rng.choice(pidx.shape[0], size=min(40, pidx.shape[0]), replace=False)
    checked = 0
    for ri in rays:
        for s in range(pidx.shape[1]):
            ids = pidx[ri, s]
            v = ids[ids >= 0]
            if v.size == 0:
                continue
            assert np.all(ids[v.size:] == -1)                 # -1 only as a suffix
            assert len(set(v.tolist())) == v.size             # no duplicates
            d = xn[v] - loc[ri, s]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert np.all(d2.astype(np.float32) <= np.float32(r) * np.float32(r))
            bidx, _, n = oq.bruteforce(xn, loc[ri, s], r)
            assert np.isin(v, bidx).all()
            checked += 1
    assert checked > 50


def test_threads_do_not_change_results():
    opt, xyz, inp = _scene(4, 2000, SR=24)
    _same(pyref.query(opt, xyz, inp, nthreads=1), pyref.query(opt, xyz, inp, nthreads=4))


def test_overflow_is_reported():
    opt, xyz, inp = _scene(1, 4000, radius=0.02, P=2)
    q = pyref.query(opt, xyz, inp)
    assert q["info"]["ovf_P"] == 1 and q["info"]["max_cnt"] > 2


if __name__ == "__main__":
    # rewrite tests/golden/ref_query.npz from the reference's kernels (oracle/_ref: needs the reference checkout to build)
    assert oq.have_ref(), "the reference's kernels (oracle/_ref) are not available here"
    oq.build()
    _RECORD = {}
    for sc in SCENES:
        test_oracle_equals_reference_kernels(*sc)
    test_config1_chair_equals_reference_kernels()
    test_edge_cases_match_reference()
    for name in query_case.REF_NAMES:
        test_query_cases_equal_reference_kernels(name)
    out = {}
    for case, r in _RECORD.items():
        out.update({case + "/sample_pidx": r["sample_pidx"].numpy(), case + "/sample_loc_w": r["sample_loc_w"].numpy(),
                    case + "/ray_mask": r["ray_mask"].numpy(), case + "/curand_hits": np.array(r["info"]["curand_hits"], np.int64)})
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d cases, %d bytes" % (GOLDEN, len(_RECORD), os.path.getsize(GOLDEN)))

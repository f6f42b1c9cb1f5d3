"""GPU tests of the fused probe pass (pointnerf_amd/csrc/probe.hip; ``fused_probe`` of the ray marcher; probe.probe_hole(fused=True)):
  (a) the synthetic ray and mask cases of tests/probe_case.py on the device, against the torch restatement and both statements of the rule;
  (b) the ray marcher with ``opt.prob == 1`` on a real render, fused against unfused: the forward is bit-reproducible
      (tests/test_gpu_reproducible.py), so both see identical opacities and weights, the selection cannot flip and every probe output must
      agree to the bars of the synthetic cases;
  (c) ``probe_hole`` end to end, fused against unfused: same candidates in the same order, the five returned tensors to those bars;
  (d) two processed views around one that hits nothing: skipped, ``prob_mul`` once per processed view, like the unfused path.
The comparison of the probe outputs with the CPU oracle stays in tests/test_gpu_level1.py / test_gpu_model_shell.py (the unfused form)."""
import numpy as np
import pytest
import torch

import probe_case as C
from cases import CASES
from oracle import pyref
from pointnerf_amd import config, ops, probe, scenes
from pointnerf_amd.mvs_points_volumetric_model import create_model
from pointnerf_amd.neural_points_volumetric_model import PROBE_KEYS, fill_invalid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
H = W = 800
SIZE = 44                    # the 0.06-radius cloud covers ~17 px around the image centre: hits inside, misses around (test_gpu_model_shell.py)
PROB_MUL = 0.4


# ---------------------------------------------------------------------------------------------------- (a) synthetic cases
@pytest.mark.parametrize("near0", [True, False])
@pytest.mark.parametrize("R,SR,K", C.RAY_CASES)
def test_probe_rays_match_the_restatement(R, SR, K, near0):
    pts, c = C.points(near0), C.ray_case(R, SR, K)
    ref, scale = C.restate(pts, c)
    dp = {k: v.to(DEV).contiguous() for k, v in pts.items()}
    P = ops.make_points(dp["xyz"], dp["points_embeding"], dp["points_conf"], dp["points_dir"], dp["points_color"])
    d = {k: v.to(DEV) for k, v in c.items()}
    got = ops.probe_rays(P, d["opacity"], d["weight"], d["sample_loc"], d["sample_pidx"], d["ray_hit"], R, SR, K)
    got = {k: v.cpu() for k, v in got.items()}
    C.check(got, ref, scale, "R%d SR%d K%d near0=%d" % (R, SR, K, near0))
    for r in range(3, R, 4):                                  # the rays that missed: exact zeros although their input rows are NaN
        assert all(float(got[k][r].abs().max()) == 0.0 for k in C.KEYS)


@pytest.mark.parametrize("far_thresh", [-1.0, C.FAR_THRESH])
@pytest.mark.parametrize("Hm,Wm", C.MASK_CASES)
def test_hole_mask_equals_both_statements_of_the_rule(Hm, Wm, far_thresh):
    c = {k: v.to(DEV) for k, v in C.mask_case(Hm, Wm).items()}
    aten, loops = C.mask_references(c, far_thresh)
    flags = ops.probe_hole_flags(c["ray_mask"], c["ray_max_shading_opacity"], c["ray_max_far_dist"], c["coarse_raycolor"], c["gt"], c["edge"],
                                 c["bg"], C.OPACITY_THRESH, far_thresh)
    got = flags.cpu().numpy() > 0
    assert np.array_equal(got, aten) and np.array_equal(got, loops), (got.astype(int), aten.astype(int), loops.astype(int))
    cand, counters = ops.compact_valid(flags.reshape(-1))
    n = int(counters[0])
    assert n == int(got.sum()) and np.array_equal(cand[:n].cpu().numpy(), np.nonzero(got.reshape(-1))[0])


# ---------------------------------------------------------------------------------------------------- the real render
@pytest.fixture(scope="module")
def shell(tmp_path_factory):
    """the `small_k8` scene in the model shell, the 44 x 44 block around the image centre, and both forms of the ray marcher's prob == 1 output"""
    ov, n, _, seed = CASES["small_k8"]
    opt = config.lego_train_opt(**ov, gpu_ids=[0], checkpoints_dir=str(tmp_path_factory.mktemp("probe")), num_point=n, default_conf=-1.0,
                                is_train=0, prob_mul=PROB_MUL, prob_num_step=1)
    xyz = torch.from_numpy(scenes.chair_points(n, seed=seed, radius=0.06))
    attrs = {k: torch.from_numpy(v) for k, v in scenes.point_attributes(n, opt.point_features_dim, seed).items()}
    m = create_model(opt)
    m.aggregator.load_state_dict(pyref.init_mlp_params(opt, seed=seed, bias_scale=0.1))
    m.aggregator.flatten_()
    a = {k: v.to(DEV) for k, v in attrs.items()}
    m.set_points(xyz.to(DEV), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"])
    inp = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=400 - SIZE // 2, y0=400 - SIZE // 2, size=SIZE))
    off = pyref.to_torch_inputs(scenes.block_rays(theta_deg=30.0, x0=20, y0=20, size=SIZE))          # the block shifted off the cloud
    rm = m.net_ray_marching
    m.set_input({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()})
    m.opt.prob = 1
    try:
        with torch.no_grad():
            raw_u = rm(**m.input)
            dense = {k: m.neural_points.querier.last_dense[k].clone() for k in ("sample_loc", "sample_pidx", "ray_hit")}
            rm.fused_probe = True
            raw_f = rm(**m.input)
            assert all(torch.equal(dense[k], m.neural_points.querier.last_dense[k]) for k in dense)
            full_u = fill_invalid(raw_u, m.input["bg_color"], prob=1)
            full_f = fill_invalid(raw_f, m.input["bg_color"], prob=1)
    finally:
        rm.fused_probe = False
        m.opt.prob = 0
    # the restatement on the unfused form's compacted tensors (every row a hit ray): the exact averages and the bars' sum_k |w_k row_k|
    hit = dense["ray_hit"].cpu() > 0
    pts = dict(xyz=xyz, **{k: v.reshape(-1, v.shape[-1]) for k, v in attrs.items()})
    comp = dict(opacity=raw_u["coarse_point_opacity"][0].cpu(), weight=raw_u["weight"][0].cpu(), sample_loc=dense["sample_loc"].cpu()[hit],
                sample_pidx=dense["sample_pidx"].cpu()[hit], ray_hit=torch.ones(int(hit.sum()), dtype=torch.int32))
    ref, scale = C.restate(pts, comp)
    return dict(opt=opt, m=m, inp=inp, off=off, raw_u=raw_u, raw_f=raw_f, full_u=full_u, full_f=full_f, hit=hit, ref=ref, scale=scale)


def test_fused_probe_outputs_equal_the_unfused_ones_on_a_real_render(shell):
    raw_u, raw_f, full_u, full_f, hit = (shell[k] for k in ("raw_u", "raw_f", "full_u", "full_f", "hit"))
    R = hit.numel()
    assert R == SIZE * SIZE and 50 < int(hit.sum()) < R - 50
    assert "_dense_probe" in raw_f and "_dense_color" in raw_f and "_hit_index" not in raw_f
    assert not any(k in raw_f for k in ("weight", "blend_weight", "conf_coefficient"))
    assert "weight" in raw_u and "conf_coefficient" in raw_u and "_dense_probe" not in raw_u          # the default form is what it was
    assert torch.equal(raw_u["ray_mask"], raw_f["ray_mask"])
    for k in ("coarse_raycolor", "coarse_point_opacity", "coarse_is_background"):
        assert torch.equal(full_u[k], full_f[k]), k
    fused, unfused = {}, {}
    for k in PROBE_KEYS:
        a, b = full_f[k].cpu(), full_u[k].cpu()
        assert a.shape == b.shape == (1, R, b.shape[-1]) and a.dtype == torch.float32, (k, a.shape, b.shape)
        assert float(a[0][~hit].abs().max()) == 0.0 and float(b[0][~hit].abs().max()) == 0.0, k
        fused[k], unfused[k] = a[0][hit], b[0][hit]
    C.check(fused, unfused, shell["scale"], "fused vs unfused")
    C.check(fused, shell["ref"], shell["scale"], "fused vs restatement")


def _threshold(shell):
    """in the widest gap of the rendered maxima (random-init MLP: they are all ~1e-3), so that no comparison sits on the threshold"""
    op = np.sort(shell["full_u"]["ray_max_shading_opacity"][0, :, 0].cpu().numpy()[shell["hit"].numpy()])
    gaps = np.diff(op)
    lo = len(op) // 4
    j = lo + int(np.argmax(gaps[lo:3 * len(op) // 4]))
    thresh = float(0.5 * (op[j] + op[j + 1]))
    assert gaps[j] > 1e-3 * thresh
    return thresh


def _candidate_scales(shell, mask):
    """rows of the bars' sum_k |w_k row_k| for the candidates of the centre view, in candidate (row-major pixel) order"""
    pix = shell["inp"]["pixel_idx"].reshape(-1, 2).long()
    ray_of = torch.full((H * W,), -1, dtype=torch.long)
    ray_of[pix[:, 1] * W + pix[:, 0]] = torch.arange(pix.shape[0])
    rays = ray_of[torch.nonzero(mask.reshape(-1)).squeeze(1)]
    assert bool((rays >= 0).all()) and bool(shell["hit"][rays].all())
    rank = (torch.cumsum(shell["hit"].long(), 0) - 1)[rays]
    return {k: v[rank] for k, v in shell["scale"].items()}


def _check_added(got_f, got_u, scales, conf_factor):
    names = ("ray_max_sample_loc_w", "shading_avg_embedding", "shading_avg_color", "shading_avg_dir", "shading_avg_conf")
    for a, b, k in zip(got_f, got_u, names):
        a, b = a.cpu(), b.cpu()
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k == "ray_max_sample_loc_w":
            assert torch.equal(a, b)                                   # a selection: bit-equal, and with it the candidates' order
        else:
            bar = 2e-6 * scales[k] * (conf_factor if k == "shading_avg_conf" else 1.0) + 1e-30
            assert bool(((a.double() - b.double()).abs() <= bar).all()), (k, float(((a.double() - b.double()).abs() / bar).max()))


def test_probe_hole_fused_equals_unfused_end_to_end(shell):
    m, opt = shell["m"], shell["opt"]
    thresh = _threshold(shell)
    view = dict(shell["inp"], id=0)
    qs = opt.query_size
    seen = {}
    got_u = probe.probe_hole(m, [view], opt, H, W, test_steps=0, opacity_thresh=thresh, frame_ids=[0], chunk=700,
                             on_view=lambda i, maps, mk: seen.setdefault("u", mk.cpu()))
    assert not getattr(m.net_ray_marching, "fused_probe", False)
    got_f = probe.probe_hole(m, [view], opt, H, W, test_steps=0, opacity_thresh=thresh, frame_ids=[0], chunk=700, fused=True,
                             on_view=lambda i, maps, mk: seen.setdefault("f", mk.cpu()))
    assert opt.prob == 0 and opt.no_loss == 0 and opt.query_size is qs and m.net_ray_marching.fused_probe is False
    n = got_u[0].shape[0]
    assert 5 < n < int(shell["hit"].sum()) and got_f[0].shape[0] == n
    assert seen["f"].dtype == torch.bool and seen["f"].shape == (H, W) and torch.equal(seen["f"], seen["u"]) and int(seen["f"].sum()) == n
    assert got_f[1].shape == (n, 32) and got_f[4].shape == (n, 1)
    _check_added(got_f, got_u, _candidate_scales(shell, seen["u"]), PROB_MUL)


def test_probe_hole_fused_skips_a_view_without_hits_like_the_unfused_path(shell):
    m, opt = shell["m"], shell["opt"]
    thresh = _threshold(shell)
    views = [dict(shell["inp"], id=0), dict(shell["off"], id=1)]
    got, order = {}, {}
    for fused in (False, True):
        order[fused] = []
        got[fused] = probe.probe_hole(m, views, opt, H, W, test_steps=0, opacity_thresh=thresh, frame_ids=[0, 1, 0], chunk=700, fused=fused,
                                      on_view=lambda i, maps, mk, f=fused: order[f].append((i, mk.cpu())))
    assert [i for i, _ in order[True]] == [i for i, _ in order[False]] == [0, 0]                    # the view that hits nothing is skipped
    mask = order[False][0][1]
    n = int(mask.sum())
    assert n > 5 and got[True][0].shape[0] == got[False][0].shape[0] == 2 * n and all(torch.equal(mk, mask) for _, mk in order[True])
    one = _candidate_scales(shell, mask)
    scales = {k: torch.cat([v, v]) for k, v in one.items()}
    factor = torch.cat([torch.full((n, 1), PROB_MUL * PROB_MUL), torch.full((n, 1), PROB_MUL)]).double()
    _check_added(got[True], got[False], scales, factor)
    # prob_mul once per PROCESSED view: the first view's candidates were scaled twice, the skipped view scaled nothing
    conf = got[True][4].cpu()
    assert bool(((conf[:n].double() - conf[n:].double() * PROB_MUL).abs() <= 4 * C.EPS * conf[:n].abs().double() + 1e-30).all())
    assert opt.prob == 0 and opt.no_loss == 0 and m.net_ray_marching.fused_probe is False

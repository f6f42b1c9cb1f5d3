"""Depth and mask supervision on the device (tests/geometry_grad_case.py).

Kernel alone: pnerf_raymarch_backward_geom on raymarch_case's cases with a seeded per-slot depth and per-ray geometry gradients, geometry
alone and with a colour gradient, per ray against the float64 autograd: the kernel's median / p95 / max of E at most 2 x the fp32
autograd's (opaque: E <= 2e-5 where the autograd is within 1e-5).  Bit conditions: zero grad_geom gives pnerf_raymarch_backward's values,
d rgb unchanged, power-of-two scales, a ray alone, guarded memory, NaN depths on invalid slots, two calls; the return codes.
Loss pass: ops.GeometryLossRays against a float64 numpy statement within derived bounds.
Through the model: small_k4 with geometry_grad against oracle/pyref.py (values at the forward bar 1e-4, gradients within the bars of
tests/test_gpu_backward.py::_check), the chunk-by-chunk recompute against the one-pass route, three optimize_parameters steps of the shell
with both items, and the shell with the items empty against a shell that never heard of them."""
import numpy as np
import pytest
import torch

import geometry_grad_case as G
import raymarch_case as RC
from cases import CASES, build_case
from gpu_util import DEV
from test_gpu_backward import _check

pytestmark = pytest.mark.gpu
_runs = {}
CASE_VARIANTS = [(c, v) for c in RC.CASES for v in G.VARIANTS]
_id = lambda cv: "%s-%s" % (RC.case_id(cv[0]), cv[1])


def _run(case, variant):
    key = (case, variant)
    if key not in _runs:
        _runs[key] = G.hip_backward_geom(G.reference(case, variant), DEV)
    return _runs[key]


@pytest.mark.parametrize("cv", CASE_VARIANTS, ids=_id)
def test_geometry_backward_per_ray_against_float64(cv):
    G.check_backward(G.reference(*cv), _run(*cv))


@pytest.mark.parametrize("cv", CASE_VARIANTS, ids=_id)
def test_rgb_gradient_unchanged_invalid_slots_and_two_calls(cv):
    ref = G.reference(*cv)
    G.check_rgb_unchanged_and_invalid_slots(ref, _run(*cv), DEV)
    assert torch.equal(G.hip_backward_geom(ref, DEV), _run(*cv)), (cv, "two calls, different gradient bits")


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_zero_geometry_gradient_is_the_existing_backward(case):
    G.check_zero_geom_is_plain(G.reference(case, "both"), DEV)


@pytest.mark.parametrize("SR", RC.SRS)
@pytest.mark.parametrize("variant", G.VARIANTS)
def test_gradient_scales_by_exact_powers_of_two(SR, variant):
    G.check_scaling(G.reference(("thin", SR, "white"), variant), DEV)


@pytest.mark.parametrize("case", [("thin", 65, "white"), ("opaque", 65, "white"), ("mixed", 130, "none"), ("opaque", 160, "white")], ids=RC.case_id)
def test_ray_alone_guarded_memory_and_poisoned_depths(case):
    ref = G.reference(case, "both")
    grad = _run(case, "both")
    for r in (0, ref.base.rows["surface"][-1], RC.R - 1):
        G.check_ray_alone(ref, grad, DEV, r)
    G.check_guarded_memory(ref, grad, DEV)
    G.check_poisoned_z(ref, grad, DEV)


def test_return_codes():
    G.check_return_codes(DEV)
    G.check_render_backward_geom_return_codes(DEV)


@pytest.mark.parametrize("mask_kind", G.MASKS)
def test_loss_pass_against_float64(mask_kind):
    G.check_loss_pass(mask_kind, DEV)


# ---- through the model ------------------------------------------------------------------------------------------------------------------------
_model = {}


def _model_runs():
    """the oracle's step and the device's one-pass step on small_k4, computed once"""
    if not _model:
        case = build_case(G.MODEL_CASE)
        R = case[3]["raydir"].shape[1]
        gt_depth, gt_mask = G.supervision(R)
        _model.update(case=case, sup=(gt_depth, gt_mask), oracle=G.oracle_step(case, gt_depth, gt_mask), hip=G.model_step(case, DEV, gt_depth, gt_mask))
    return _model


def test_model_geometry_values_match_the_oracle():
    m = _model_runs()
    (ov, _), (hv, _) = m["oracle"], m["hip"]
    for k in ("acc", "T"):
        assert float((hv[k] - ov[k]).abs().max()) <= 1e-4, k
    depth = hv["depth_sum"] / (hv["acc"] + 1e-6)
    e = float((depth - ov["depth"]).abs().max())
    print("depth: max |hip - oracle| %.2e over %d hit rays; L_depth %.6g / %.6g, L_bg %.6g / %.6g" % (e, depth.numel(), hv["l_depth"], float(ov["l_depth"]),
                                                                                                    hv["l_bg"], float(ov["l_bg"])))
    assert e <= 1e-4
    assert float(ov["l_depth"]) > 0 and float(ov["l_bg"]) > 0
    assert abs(hv["l_depth"] - float(ov["l_depth"])) <= 1e-4 * float(ov["l_depth"]) and abs(hv["l_bg"] - float(ov["l_bg"])) <= 1e-4 * float(ov["l_bg"])


def test_model_gradients_match_the_oracle():
    m = _model_runs()
    (_, og), (_, hg) = m["oracle"], m["hip"]
    assert set(og) == set(hg)
    for k in og:
        _check(k, hg[k].reshape(og[k].shape), og[k])


def test_geometry_terms_reach_the_gradients():
    """the geometry terms are really in the gradient: without them (colour / zero-one loss alone) it differs by far more than the bars"""
    from oracle import pyref
    m = _model_runs()
    model, agg, npnt, d = G.build_trainable(m["case"], DEV, geometry_grad=False)
    out = model(**d)
    assert "_dense_geometry" not in out
    pyref.training_loss(m["case"][0], out, {"gt_image": d["gt_image"]}).backward()
    plain = npnt.points_embeding.grad.detach().cpu()
    with_geo = m["hip"][1]["points_embeding"]
    assert float((with_geo - plain).abs().max()) > 0.05 * float(with_geo.abs().max())


def test_chunked_recompute_equals_one_pass(monkeypatch):
    """the chunk-by-chunk recompute (fused._backward_in_chunks slices grad_geom per chunk) under the tolerance of
    tests/test_gpu_backward.py::_chunked_equals_one_pass"""
    from pointnerf_amd.fused import FusedRender
    m = _model_runs()
    one = m["hip"][1]
    monkeypatch.setenv("PNERF_ARENA_BUDGET_GB", "0.002")
    FusedRender.last_chunks = None
    _, many = G.model_step(m["case"], DEV, *m["sup"])
    assert FusedRender.last_chunks is not None and FusedRender.last_chunks[0] < FusedRender.last_chunks[1], "the budget did not force chunks"
    for k in one:
        scale = max(float(one[k].abs().max()), 1e-12)
        assert float((one[k] - many[k]).abs().max()) <= 2e-5 * scale, k


def _shell(tmp_path, drop=(), **kw):
    from pointnerf_amd import config, scenes
    from pointnerf_amd.mvs_points_volumetric_model import create_model
    from oracle import pyref
    ov, n, size, seed = CASES[G.MODEL_CASE]
    opt = config.lego_train_opt(**ov, gpu_ids=[0], checkpoints_dir=str(tmp_path), num_point=n, default_conf=-1.0, ray_jitter=0.0, **kw)
    for name in drop:                                   # options that have never heard of the items
        delattr(opt, name)
    opt, xyz, attrs, inp, mlp = (opt,) + build_case(G.MODEL_CASE)[1:]
    m = create_model(opt)
    m.aggregator.load_state_dict(mlp)
    m.aggregator.flatten_()
    a = {k: v.to(DEV) for k, v in attrs.items()}
    m.set_points(xyz.to(DEV), a["points_embeding"], points_color=a["points_color"], points_dir=a["points_dir"], points_conf=a["points_conf"])
    m.setup(opt)
    m.train()
    return opt, m, (xyz, attrs, inp, mlp)


def _steps(m, inp, n, extra):
    seen = []
    for step in range(n):
        data = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
        data.update({k: v.clone() for k, v in extra.items()})
        data["id"] = torch.tensor([3])
        m.set_input(data)
        m.optimize_parameters(total_steps=step)
        seen.append({k: float(v) for k, v in m.get_current_losses().items()})
    return seen


def test_shell_three_steps_with_both_items(tmp_path):
    from oracle import pyref
    opt, m, (xyz, attrs, inp, mlp) = _shell(tmp_path, depth_loss_items=["coarse_depth"], depth_loss_weights=[G.W_DEPTH],
                                            bg_loss_items=["coarse_is_background"], bg_loss_weights=[G.W_BG])
    assert m.net_ray_marching.geometry_grad is True
    R = inp["raydir"].shape[1]
    gt_depth, gt_mask = G.supervision(R)
    with torch.no_grad():
        ref = G.oracle_geometry_losses(pyref.render(opt, dict(xyz=xyz, **attrs), mlp, inp, nthreads=8), gt_depth, gt_mask)
    with pytest.raises(RuntimeError, match="gt_depth"):
        _steps(m, inp, 1, dict(gt_mask=gt_mask))
    with pytest.raises(RuntimeError, match="gt_mask"):
        _steps(m, inp, 1, dict(gt_depth=gt_depth))
    seen = _steps(m, inp, 3, dict(gt_depth=gt_depth, gt_mask=gt_mask))
    print("step 0: loss_coarse_depth %.6g (oracle %.6g), loss_coarse_is_background %.6g (oracle %.6g)"
          % (seen[0]["coarse_depth"], float(ref["l_depth"]), seen[0]["coarse_is_background"], float(ref["l_bg"])))
    assert abs(seen[0]["coarse_depth"] - float(ref["l_depth"])) <= 1e-4 * float(ref["l_depth"])
    assert abs(seen[0]["coarse_is_background"] - float(ref["l_bg"])) <= 1e-4 * float(ref["l_bg"])
    for s in seen:
        assert all(np.isfinite(v) for v in s.values()), s
        assert {"total", "coarse_depth", "coarse_is_background"} <= set(s)
    assert "_dense_geometry" in m._raw and "_dense_color" in m._raw           # the fused colour loss stays on, next to the geometry terms
    assert seen[2]["coarse_depth"] != seen[0]["coarse_depth"]                 # the parameters moved
    out = m.test()                                                             # a no-grad pass of the same shell computes the same terms
    assert np.isfinite(float(m.loss_coarse_depth)) and not out["coarse_raycolor"].requires_grad


def test_shell_with_empty_items_is_the_shell_without_the_option(tmp_path):
    """items empty: the first step -- every loss value, the filled image, and the weight gradients the backward forms without atomics
    (tests/test_gpu_reproducible.py) -- has the bits of a shell whose options never named the items.  (Later steps are not comparable bit
    for bit even between two runs of ONE shell: the point gradients are atomic sums.)"""
    runs = []
    names = ("depth_loss_items", "depth_loss_weights", "bg_loss_items", "bg_loss_weights")
    for i, kw in enumerate((dict(drop=names), dict(depth_loss_items=[], bg_loss_items=[], depth_loss_weights=[1.0], bg_loss_weights=[1.0]))):
        opt, m, (xyz, attrs, inp, mlp) = _shell(tmp_path / str(i), **kw)
        assert m.net_ray_marching.geometry_grad is False
        seen = _steps(m, inp, 1, {})
        assert "_dense_geometry" not in m._raw
        det = {n: p.grad.detach().clone() for n, p in m.aggregator.named_parameters()
               if n in ("block1.0.weight", "block1.2.weight", "block3.0.weight", "block3.2.weight", "color_branch.0.weight", "color_branch.2.weight",
                        "color_branch.4.weight")}
        runs.append((seen[0], sorted(m._raw), m.output["coarse_raycolor"].detach().clone(), det))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    assert len(a[3]) == 7
    for k in a[3]:
        assert float(a[3][k].abs().max()) > 0 and torch.equal(a[3][k], b[3][k]), k

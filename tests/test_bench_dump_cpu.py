"""bench.py --dump-outputs on host tensors: which arrays it writes, in which dtype, and the fixed row sample of the per-point tensors."""
import os

import numpy as np
import torch

import bench


def _params(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    mlp = [("block1.0.weight", torch.nn.Parameter(torch.randn(4, 3, generator=g))), ("block1.0.bias", torch.nn.Parameter(torch.randn(4, generator=g)))]
    pts = [("points_embeding", torch.nn.Parameter(torch.randn(1, n, 5, generator=g))), ("points_conf", torch.nn.Parameter(torch.rand(1, n, 1, generator=g)))]
    for _, p in mlp + pts:
        p.grad = torch.randn(p.shape, generator=g)
    return mlp, pts


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_of_the_fused_training_output(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_POINT_ROWS", 16)
    n, R = 40, 10
    mlp, pts = _params(n)
    hit = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 0, 1], dtype=torch.int32)
    color = torch.rand(R, 3)
    out = {"_dense_color": (color, hit, int(hit.sum())), "ray_mask": (hit > 0).to(torch.int8)[None]}
    names = bench.dump_outputs(str(tmp_path / "a"), out, torch.tensor(0.25), mlp, pts)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == names
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["loss"].tolist() == [0.25]
    assert np.array_equal(got["coarse_raycolor"], color[hit > 0].numpy()) and np.array_equal(got["ray_mask"], (hit > 0).float().numpy())
    assert np.array_equal(got["mlp.block1.0.weight"], mlp[0][1].detach().numpy()) and np.array_equal(got["mlp_grad.block1.0.bias"], mlp[1][1].grad.numpy())
    rows = np.sort(np.random.default_rng(bench.DUMP_ROW_SEED).choice(n, 16, replace=False))
    assert np.array_equal(got["points_embeding"], pts[0][1].detach()[0].numpy()[rows])
    assert np.array_equal(got["points_conf_grad"], pts[1][1].grad[0].numpy()[rows])
    assert got["points_grad_abs_sum"].dtype == np.float64
    assert np.allclose(got["points_grad_abs_sum"], [float(p.grad.double().abs().sum()) for _, p in pts])
    # the same point count selects the same rows
    bench.dump_outputs(str(tmp_path / "b"), out, torch.tensor(0.25), mlp, pts)
    assert all(np.array_equal(v, _load(str(tmp_path / "b"))[k]) for k, v in got.items())


def test_dump_of_the_compacted_output_keeps_every_row_of_a_small_cloud(tmp_path):
    mlp, pts = _params(12, seed=1)
    out = {"coarse_raycolor": torch.rand(1, 2, 3), "ray_mask": torch.tensor([[0, 1, 1]], dtype=torch.int8)}
    bench.dump_outputs(str(tmp_path), out, torch.tensor(1.5), mlp, pts)
    got = _load(str(tmp_path))
    assert np.array_equal(got["coarse_raycolor"], out["coarse_raycolor"][0].numpy())
    assert np.array_equal(got["points_embeding"], pts[0][1].detach()[0].numpy())
    # render only: no parameters, no gradients
    bench.dump_outputs(str(tmp_path / "r"), out, torch.tensor(1.5), [], [])
    assert sorted(os.listdir(str(tmp_path / "r"))) == ["coarse_raycolor.npy", "loss.npy", "ray_mask.npy"]


def _adam(p, g, m, v, lr, b1, b2, eps, step):          # torch.optim.Adam's update, the restatement FusedAdam takes on the host
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    p.sub_(lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps))


def test_reset_training_state_makes_the_next_step_a_first_step():
    """the last timed step starts from the seeded initial state: after some steps and the reset, one step equals one step of a fresh optimizer"""
    from pointnerf_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(7, 5, generator=g), torch.randn(11, generator=g)]
    grads = [[torch.randn(t.shape, generator=g) for t in init] for _ in range(4)]

    def run(params, opt, gs):
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        opt.step()

    ps = [torch.nn.Parameter(t.clone()) for t in init]
    o = FusedAdam(ps, lr=0.01, update=_adam)
    for k in range(3):
        run(ps, o, grads[k])
    assert not torch.equal(ps[0].detach(), init[0])
    addr = [p.data_ptr() for p in ps] + [o.state[p]["exp_avg"].data_ptr() for p in ps]
    bench.reset_training_state(ps, [t.clone() for t in init], [o])
    assert all(torch.equal(p.detach(), t) for p, t in zip(ps, init))
    run(ps, o, grads[3])
    fresh = [torch.nn.Parameter(t.clone()) for t in init]
    run(fresh, FusedAdam(fresh, lr=0.01, update=_adam), grads[3])
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(ps, fresh))
    assert addr == [p.data_ptr() for p in ps] + [o.state[p]["exp_avg"].data_ptr() for p in ps]        # in place


def test_reset_training_state_of_the_sharded_optimizer():
    """--zero1 runs: ShardedAdam's step count and flat moments are reset as well (one rank, no process group: its update runs locally)"""
    from pointnerf_amd.optim import ShardedAdam
    g = torch.Generator().manual_seed(4)
    init = [torch.randn(6, 3, generator=g), torch.randn(5, generator=g)]
    grads = [[torch.randn(t.shape, generator=g) for t in init] for _ in range(3)]

    def run(params, opt, gs):
        for p, gr in zip(params, gs):
            p.grad = gr.clone()
        opt.step()

    ps = [torch.nn.Parameter(t.clone()) for t in init]
    o = ShardedAdam(ps, lr=0.01, update=_adam)
    for k in range(2):
        run(ps, o, grads[k])
    assert o.step_count == 2 and float(o.exp_avg.abs().sum()) > 0
    addr = (o.flat_param.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr())
    bench.reset_training_state(ps, [t.clone() for t in init], [o])
    assert o.step_count == 0 and not o.exp_avg.any() and not o.exp_avg_sq.any()
    assert all(torch.equal(p.detach(), t) for p, t in zip(ps, init))
    run(ps, o, grads[2])
    fresh = [torch.nn.Parameter(t.clone()) for t in init]
    run(fresh, ShardedAdam(fresh, lr=0.01, update=_adam), grads[2])
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(ps, fresh))
    assert addr == (o.flat_param.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr())

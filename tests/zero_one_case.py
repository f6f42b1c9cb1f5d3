"""The unified zero-one pass (one forward / one backward kernel over rows x slots, csrc/loss.hip) in its two forms -- the flat index list
(ops.zero_one_conf_sum) and the dense neighbor table with hit flags (ops.zero_one_conf_sum_rays) -- against the ATen chain it replaces:
gather with the -1 -> point 0 rule, gradient_clamp, clamp(eps, 1 - eps), log + log(1 - .), sum.  Shared by the emulator test
(tests/test_emu_kernels.py) and the device test (tests/test_gpu_level1.py): same shapes, each with the bars of its neighbour test there.

Shapes, each the smallest that reaches a distinct loop path of the kernels (256 threads per workgroup, a workgroup per row at a time):
  flat  n_idx = 6000           24 rows, the last one 112 long
  rays  R = 37, slots = 192    fewer slots than threads; about half the rays missed, ray 0 and ray R - 1 among them
  rays  R = 5,  slots = 300    a second trip of the inner loop
"""
import functools

import torch

from pointnerf_amd import ops
from pointnerf_amd.neural_points_volumetric_model import gradient_clamp

N, EPS, GSCALE = 500, 1e-3, 0.37
SHAPES = {"flat_6000": (None, 6000), "rays_37x192": (37, 192), "rays_5x300": (5, 300)}


@functools.lru_cache(maxsize=None)
def case(name):
    """(conf [1,N,1], pidx [n] or [R,slots] int32, ray_hit [R] int32 or None, reference value, reference conf gradient); read-only"""
    R, slots = SHAPES[name]
    g = torch.Generator().manual_seed(3 + slots)
    conf = torch.rand(1, N, 1, generator=g) * 1.2 - 0.1                 # some below 1e-4 / eps, some above 1 - eps and above 1
    conf[0, :5, 0] = torch.tensor([0.0, 1e-4, 1e-3, 1 - 1e-3, 1.0])     # the clamp bounds themselves
    shape = (slots,) if R is None else (R, slots)
    pidx = torch.randint(-1, N, shape, generator=g, dtype=torch.int32)
    pidx[torch.rand(shape, generator=g) < 0.4] = -1                     # empty slots: the point-0 flood
    hit = None
    if R is not None:
        hit = (torch.rand(R, generator=g) < 0.5).to(torch.int32) * 3    # (any positive number is a hit)
        hit[0] = hit[R - 1] = 0
        hit[1] = 1
    ref, grad = reference(conf, pidx if hit is None else pidx[hit > 0])
    return conf, pidx, hit, ref, grad


def reference(conf, pidx):
    a = conf.clone().requires_grad_(True)
    cc = gradient_clamp(a.reshape(-1)[pidx.reshape(-1).long().clamp(min=0)])
    v = cc.clamp(EPS, 1 - EPS)
    ref = (torch.log(v) + torch.log(1 - v)).sum()
    (ref * GSCALE).backward()
    return ref.detach(), a.grad


def run(conf, pidx, hit, dev):
    """(sum, conf gradient) of the fused pass on ``dev``, brought back to the host"""
    b = conf.to(dev).clone().requires_grad_(True)
    if hit is None:
        got = ops.zero_one_conf_sum(b, pidx.to(dev), EPS)
    else:
        got = ops.zero_one_conf_sum_rays(b, pidx.to(dev), hit.to(dev), EPS)
    (got * GSCALE).backward()
    return got.detach().cpu(), b.grad.cpu()


def check_against_the_chain(name, dev, close):
    """``close(value, ref_value, grad, ref_grad)`` asserts the caller's bars"""
    conf, pidx, hit, ref, grad = case(name)
    got, ggrad = run(conf, pidx, hit, dev)
    print(name, "value", float(got), "ref", float(ref), "max |grad diff|", float((ggrad - grad).abs().max()), "max |grad|", float(grad.abs().max()))
    close(got, ref, ggrad, grad)
    if hit is not None:
        # the flat form on the compacted table of the hit rays: the same elements in another thread-to-element map
        fgot, fgrad = run(conf, pidx[hit > 0].reshape(-1), None, dev)
        close(fgot, got, fgrad, ggrad)


def check_exact_conditions(dev):
    conf = case("flat_6000")[0]
    g = torch.Generator().manual_seed(11)
    pidx = torch.randint(-1, N, (24, 256), generator=g, dtype=torch.int32)
    # slots == threads, every ray hit: the two forms map threads to elements identically, and the forward has no atomics
    rays, _ = run(conf, pidx, torch.ones(24, dtype=torch.int32), dev)
    flat, _ = run(conf, pidx.reshape(-1), None, dev)
    assert torch.equal(rays, flat) and float(rays) != 0.0
    got, grad = run(conf, pidx, torch.zeros(24, dtype=torch.int32), dev)          # every ray missed
    assert float(got) == 0.0 and not bool(grad.any())
    got, grad = run(conf, torch.zeros(0, dtype=torch.int32), None, dev)           # nothing to sum
    assert float(got) == 0.0 and not bool(grad.any())

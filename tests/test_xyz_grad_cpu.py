"""Host logic of xyz_grad without a GPU: the optimiser drops the voxel-grid cache when it moves the point positions (the cache key would
still match the old cloud: FusedAdam writes through a raw pointer), ZeRO-1 refuses trainable positions with an error naming xyz_grad, and
on two gloo ranks the dense all-reduce of dist.allreduce_grads sums d xyz like the other point tensors."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

from pointnerf_amd import dist as pdist, point_query
from pointnerf_amd.optim import FusedAdam, ShardedAdam


def _adam(p, g, m, v, lr, b1, b2, eps, step):
    p.add_(g, alpha=-lr)


def _positions(n=50, seed=0):
    p = nn.Parameter(torch.randn(n, 3, generator=torch.Generator().manual_seed(seed)))
    p.pnerf_point_xyz = True               # what NeuralPoints sets on its position parameter
    return p


def test_fused_adam_drops_the_grid_cache_when_it_moves_positions():
    xyz, emb = _positions(), nn.Parameter(torch.randn(50, 32))
    for moved, params in ((False, [emb]), (True, [emb, xyz])):
        point_query._GRID_CACHE["sentinel"] = object()
        for p in params:
            p.grad = torch.ones_like(p)
        FusedAdam(params, lr=1e-2, update=_adam).step()
        assert ("sentinel" in point_query._GRID_CACHE) != moved
    point_query.clear_grid_cache()


def test_zero1_refuses_trainable_positions():
    with pytest.raises(NotImplementedError, match="xyz_grad"):
        ShardedAdam([nn.Parameter(torch.randn(8, 4)), _positions()], lr=1e-3, update=_adam)
    frozen = _positions()
    frozen.requires_grad_(False)
    ShardedAdam([nn.Parameter(torch.randn(8, 4)), frozen], lr=1e-3, update=_adam)     # xyz_grad = 0: accepted as before


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    xyz, emb = _positions(), nn.Parameter(torch.randn(50, 32, generator=torch.Generator().manual_seed(1)))
    g = torch.Generator().manual_seed(10 + rank)
    xyz.grad, emb.grad = torch.randn(50, 3, generator=g), torch.randn(50, 32, generator=g)
    pdist.allreduce_grads([], [emb, xyz])
    if rank == 0:
        torch.save(dict(xyz=xyz.grad, emb=emb.grad), out)
    torch.distributed.destroy_process_group()


def test_two_gloo_ranks_sum_the_position_gradients(tmp_path):
    out = str(tmp_path / "g.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out)
    ref = {"xyz": torch.zeros(50, 3), "emb": torch.zeros(50, 32)}
    for r in range(2):
        g = torch.Generator().manual_seed(10 + r)
        ref["xyz"] += torch.randn(50, 3, generator=g)
        ref["emb"] += torch.randn(50, 32, generator=g)
    for k in ref:
        assert torch.allclose(got[k], ref[k], atol=1e-6), k

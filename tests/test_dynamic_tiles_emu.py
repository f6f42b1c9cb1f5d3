"""tests/test_gpu_dynamic_tiles.py on the host emulator (tools/emu: the same kernel sources, every GPU thread a fiber, a returning atomicAdd):
the tile claim of the two tile kernels at its edges without a GPU -- fewer tile counts than on the device (the emulator is slow), every
grid, the three small-class cases in turn."""
import pytest
import torch

import test_gpu_backward as TB
from dynamic_tiles_case import MODES, cases_of, check_against_oracle, check_backward_twice, check_grids_agree, forced_case
from emu_util import emu_backend
from pointnerf_amd import ops


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(TB, "DEV", "cpu")
    with emu_backend(ncu=2):
        yield


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    """the saved-activation arena starts as NaN bit patterns: nothing unwritten may reach a result"""
    orig = ops.Arena.take

    def take(self, nbytes, device):
        t = orig(self, nbytes, device)
        t.fill_(0xFF)
        return t

    monkeypatch.setattr(ops.Arena, "take", take)


# (G, T): no tile; fewer tiles than workgroups; one past the backward's / the forward's static tiles; one past a claimed round
EMU = [(1, 0), (3, 2), (2, 5), (1, 4), (1, 5), (3, 13), (2, 9)]


@pytest.mark.parametrize("i", range(len(EMU)))
def test_emulated_tile_claim_at_its_edges(i):
    G, T = EMU[i]
    modes = cases_of(T)
    mode = modes[i % len(modes)]
    case, tiles = forced_case(T, mode)
    old = ops.set_tile_grid(G)
    try:
        print("G %d T %d %s tiles per class %s" % (G, T, mode, tiles))
        check_against_oracle(case, tiles)
    finally:
        ops.set_tile_grid(old)


def test_emulated_grids_agree_and_a_second_backward_claims_from_zero():
    case, tiles = forced_case(5, "small_both")
    check_grids_agree(case, tiles, grids=(1, 3))
    old = ops.set_tile_grid(2)
    try:
        check_backward_twice(case)
    finally:
        ops.set_tile_grid(old)

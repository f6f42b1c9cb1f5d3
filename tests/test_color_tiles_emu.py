"""tests/test_gpu_color_tiles.py on the host emulator (tools/emu: the same kernel sources, every GPU thread a fiber): the colour MLP kernels
at the edges of their tile loops, so that an indexing mistake in the per-wave running sums or in a workgroup's last tile shows up without a
GPU.  The emulated device has two CUs: the forward launches 4 colour workgroups, the backward 6."""
import pytest
import torch

import test_gpu_backward as TB
import test_gpu_render as TR
from color_tiles_case import TILE, check_backward, forced_case, library_count
from emu_util import emu_backend

NCU = 2
COUNTS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TILE * 2 * NCU + 1, TILE * 3 * NCU + 1]


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(TB, "DEV", "cpu")
    with emu_backend(ncu=NCU):
        yield


@pytest.fixture(autouse=True)
def _poison(monkeypatch):
    """the saved-activation arena starts as NaN bit patterns: nothing unwritten may reach a result"""
    from pointnerf_amd import ops
    orig = ops.Arena.take

    def take(self, nbytes, device):
        t = orig(self, nbytes, device)
        t.fill_(0xFF)
        return t

    monkeypatch.setattr(ops.Arena, "take", take)


@pytest.mark.parametrize("n", COUNTS)
def test_emulated_colour_kernels_at_the_tile_loop_edges(n):
    case = forced_case("small_k4", n, 120)
    assert library_count(case) == n, "the case does not have the forced number of valid samples"
    TR._compare(*case)
    check_backward(case, n)

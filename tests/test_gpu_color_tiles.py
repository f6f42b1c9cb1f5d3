"""The colour MLP kernels (k_color_forward, k_color_backward) at the edges of their tile loops: the render entry points on the seeded cases of
tests/cases.py with the number of valid samples forced (tests/color_tiles_case.py) to 1, 63, 64, 65, 129 and one sample past a full round of
the grid -- 64 x (workgroups launched) + 1, for the forward's two workgroups per CU and the backward's three.  A workgroup's running sums of
the bias / output-layer gradients are per-wave LDS sets that meet after its last tile: a wave that never sees a second tile, a last partial
tile and a workgroup with a single tile are the cases.  Bars: tests/test_gpu_render.py (1e-4 on sigma / RGB) and tests/test_gpu_backward.py
(_check)."""
import pytest
import torch

import test_gpu_backward as TB
import test_gpu_render as TR
from color_tiles_case import TILE, check_backward, forced_case
from gpu_util import hip_render

pytestmark = pytest.mark.gpu
BLOCK = 120                         # pixels per side of the candidate block: covers the object's silhouette (rays with a single valid sample)
EDGES = ["one", "tile-1", "tile", "tile+1", "two_tiles+1", "forward_grid+1", "backward_grid+1"]


def _count(edge):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return {"one": 1, "tile-1": TILE - 1, "tile": TILE, "tile+1": TILE + 1, "two_tiles+1": 2 * TILE + 1,
            "forward_grid+1": TILE * 2 * ncu + 1, "backward_grid+1": TILE * 3 * ncu + 1}[edge]


@pytest.mark.parametrize("name", ["small_k8", "small_k4"])
@pytest.mark.parametrize("edge", EDGES)
def test_colour_forward_at_the_tile_loop_edges(name, edge):
    n = _count(edge)
    case = forced_case(name, n, BLOCK)
    errs = TR._compare(*case)
    print(name, edge, n, "decoded err %.2e" % errs["decoded"])
    # two launches: the same bits
    d1, f1, _ = hip_render(*case)
    d2, f2, _ = hip_render(*case)
    assert int(d1["counters"][0].item()) == n, "the case does not have the forced number of valid samples"
    hit = d1["ray_hit"] > 0
    for k in ("decoded", "ray_color"):
        a, b = f1[k][hit], f2[k][hit]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, "two launches differ")


@pytest.mark.parametrize("name", ["small_k8", "small_k4"])
@pytest.mark.parametrize("edge", EDGES)
def test_colour_backward_at_the_tile_loop_edges(name, edge):
    """every MLP tensor and the per-point tensors (which carry d f), one plane and two: color_tiles_case.check_backward"""
    check_backward(forced_case(name, _count(edge), BLOCK), _count(edge))

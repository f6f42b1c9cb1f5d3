"""The saved-activation area and the inference workspace are each described by ONE walk (csrc/aggregate.hip: pn_saved_walk, csrc/render.hip:
agg_workspace_walk) that serves the byte count and the pointers.  Their sizes are part of the boundary (callers size arenas with them): the
tables below were recorded from the two-description form that the walk replaced and must not move.  Host code only: the emulator library and the
gfx950 library give the same numbers and neither needs a GPU."""
import pytest

from emu_util import emu_lib

# (n_valid, K) -> pnerf_agg_saved_bytes, by weight-gradient planes
CASES = [(0, 8), (1, 8), (8, 8), (9, 8), (100, 8), (1000, 4), (37, 12), (5, 1), (64, 16), (923000, 8)]
SAVED = {
    1: [2974720, 3318016, 3318016, 3946752, 8008448, 29454848, 6006528, 5316096, 8752896, 43727368192],
    2: [5104640, 5718272, 5718272, 6736128, 13890304, 50635264, 10417920, 8547840, 15326976, 76632616960],
}
# pnerf_agg_workspace_bytes: the same whatever the planes
WORKSPACE = [75630592, 75630592, 75630592, 75696896, 75763200, 76757760, 75696896, 76094720, 75696896, 1031868672]


def _hip_lib():
    from pointnerf_amd import _lib
    return _lib.lib()


@pytest.fixture(params=["emu", "hip"])
def lib(request):
    return emu_lib() if request.param == "emu" else _hip_lib()


@pytest.mark.parametrize("planes", [1, 2])
def test_saved_and_workspace_bytes_are_the_recorded_ones(lib, planes):
    old = lib.pnerf_set_wgrad_planes(planes)
    assert old in (1, 2)
    try:
        assert [lib.pnerf_agg_saved_bytes(n, K) for n, K in CASES] == SAVED[planes]
        assert [lib.pnerf_agg_workspace_bytes(n, K) for n, K in CASES] == WORKSPACE
        for n, K in ((100, 0), (100, 17), (-1, 8)):
            assert lib.pnerf_agg_saved_bytes(n, K) == 0 and lib.pnerf_agg_workspace_bytes(n, K) == 0
    finally:
        assert lib.pnerf_set_wgrad_planes(old) == planes


@pytest.mark.parametrize("planes", [1, 2])
def test_saved_bytes_do_not_decrease_with_the_capacity(planes):
    lib = emu_lib()
    old = lib.pnerf_set_wgrad_planes(planes)
    try:
        for K in (1, 3, 8, 12, 16):
            sizes = [lib.pnerf_agg_saved_bytes(n, K) for n in range(201)]
            assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])), K
            assert sizes[-1] > sizes[0], K
    finally:
        lib.pnerf_set_wgrad_planes(old)

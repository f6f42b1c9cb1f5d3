"""The dynamic tile claim of k_agg_forward / k_agg_backward (csrc/mlp_common.h) on the device, at the edges of the claim: grids of G = 1, 2, 3
workgroups (ops.set_tile_grid) and tile counts of the K-rows class around the multiples of G that the loops' look-aheads make special
(tests/dynamic_tiles_case.py), with the two small classes empty, both non-empty, and one of exactly one tile.  The saved arena is
NaN-poisoned (tests/conftest.py)."""
import pytest

from dynamic_tiles_case import cases_of, check_against_oracle, check_backward_twice, check_grids_agree, forced_case, tile_counts
from pointnerf_amd import ops

pytestmark = pytest.mark.gpu
GRID_TILES = [(G, T) for G in (1, 2, 3) for T in tile_counts(G)]


@pytest.mark.parametrize("G,T", GRID_TILES)
def test_every_tile_runs_exactly_once(G, T):
    """outputs and gradients within the oracle bars: a skipped tile shows as poison or zeros, a tile run twice doubles its rows' atomic sums"""
    for mode in cases_of(T):
        case, tiles = forced_case(T, mode)
        old = ops.set_tile_grid(G)
        try:
            print("G %d T %d %s tiles per class %s" % (G, T, mode, tiles))
            check_against_oracle(case, tiles)
        finally:
            ops.set_tile_grid(old)


@pytest.mark.parametrize("T,mode", [(5, "small_both"), (13, "small_one_tile"), (9, "small_empty")])
def test_results_do_not_depend_on_which_workgroup_runs_a_tile(T, mode):
    """G = 1, G = 3 and the default grid: the training forward (saved area with the f rows, decoded, weight, ray colour) byte-equal, the
    weight-gradient GEMMs' tensors bit-equal, atomically summed gradients within the bars"""
    case, tiles = forced_case(T, mode)
    check_grids_agree(case, tiles)


def test_a_second_backward_on_the_same_saved_area_sees_zeroed_counters():
    """Two forwards without a classification in between do not exist: pn_agg_forward_launch classifies (and with that zeroes cls_info and its
    claim counters) in front of every launch group.  The backward's counters sit behind its scale word and are zeroed with it by the
    backward's launcher: a backward repeated on one saved area claims from zero again"""
    case, tiles = forced_case(13, "small_both")
    for G in (2, 0):
        old = ops.set_tile_grid(G)
        try:
            check_backward_twice(case)
        finally:
            ops.set_tile_grid(old)

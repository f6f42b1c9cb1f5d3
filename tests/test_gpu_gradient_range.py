"""Gradient accuracy of down-weighted rays on the device (tests/range_case.py): the probe of the hit rays in the right half of the pixel block
is multiplied by 10^-k, k in {0, 2, 4, 6}; on the points only those rays touch, max |hip - f64| <= BAR x max |f64| OVER THOSE POINTS, with
the project's point-gradient bars (1e-5 with f16 cross terms in the input-gradient chain, 1e-4 with the shipped e4m3 chain); the fp32 oracle's
own figure is printed beside every HIP figure.  The other points and every MLP tensor keep the bars of tests/test_gpu_backward.py at every
k; the whole call multiplied by 2^-30 / 2^+20 gives the k = 0 result times that power (pn_scale_from_bits); a ray with a zero probe
contributes exactly zero.  Shapes: the smallest that reach every path of k_color_backward / k_agg_backward (three sample classes at K = 8, 4
and 12, the run-time-K front at K = 3, the two-plane weight-gradient instances)."""
import pytest

import range_case as RC
from gpu_util import hip_render
from pointnerf_amd import ops

pytestmark = pytest.mark.gpu
KS = (0, 2, 4, 6)
_refs = {}


def _ref(name):
    if name not in _refs:
        _refs[name] = RC.Reference(name)
        _refs[name].check_conditions()
    return _refs[name]


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("name", ["k8", "k4", "k3", "k12"])
def test_down_weighted_rays_keep_their_own_accuracy(name, bits):
    RC.run_arithmetic(_ref(name), hip_render, bits, KS)


def test_down_weighted_rays_two_plane_weight_gradients():
    """ops.set_wgrad_planes(2): the WG2 instances of both kernels (f16x3.h arithmetic everywhere, so the 1e-5 bar)"""
    old = ops.set_wgrad_planes(2)
    try:
        RC.run_arithmetic(_ref("k8"), hip_render, 16, KS, tag="two planes, f16 cross terms")
    finally:
        ops.set_wgrad_planes(old)

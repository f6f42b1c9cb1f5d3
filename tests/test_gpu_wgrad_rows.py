"""Weight-gradient accuracy per element on the device (tests/wgrad_rows_case.py): every fourth unit of the seven hidden layers muted at depth k
(its consumers' weight columns x 10^-k); every asserted element of every dW and db within 2^-9 of the float64 sum of its absolute terms in
one-plane mode, within 4 x the fp32 oracle's own figure per tensor in two-plane mode; the per-tensor bars of tests/test_gpu_backward.py against
float64 at every k.  Shapes: the "emu" block and range_case's "k4" and "k3", so that all three sample-class layouts of the backward front run
(K = 8: three classes, K = 4: two, K = 3: the run-time-K front).  k in {0, 2, 4} with the shipped e4m3 cross terms and one plane; k = 4 again with
f16 cross terms, and again with two planes."""
import pytest

import wgrad_rows_case as WR
from gpu_util import hip_render

pytestmark = pytest.mark.gpu
_refs = {}


def _ref(name, k):
    if (name, k) not in _refs:
        _refs[(name, k)] = WR.Reference(name, k)
        _refs[(name, k)].check_conditions()
        _refs[(name, k)].check_ideal()
    return _refs[(name, k)]


@pytest.mark.parametrize("k,bits,planes", [(0, 8, 1), (2, 8, 1), (4, 8, 1), (4, 16, 1), (4, 16, 2)])
@pytest.mark.parametrize("name", ["emu", "k4", "k3"])
def test_weight_gradient_rows_of_muted_units(name, k, bits, planes):
    WR.run(_ref(name, k), hip_render, bits, planes)

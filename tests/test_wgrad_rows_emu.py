"""Host-emulator twin of tests/test_gpu_wgrad_rows.py (tests/wgrad_rows_case.py): every element of the weight and bias gradients against float64,
relative to the float64 sum of its absolute terms, with every fourth hidden unit muted at depth k.  The emulator shares the formats, scales and
quantisation code with the device and differs in accumulation order only; an emulated backward of this size takes ~25 s, hence the "emu" case in
one-plane mode with the shipped e4m3 cross terms at k in {0, 4} only.

Before the hidden units' column scales (csrc/mixq.h) this test failed at k = 4 and passed at k = 0.  Its output there, max E / A of the muted rows | of
the other rows (bar 1.95e-3; the fp32 oracle <= 1.1e-4, the exact-sum restatement of the format <= 8.6e-4):
    block1.0  dW 4.2e-01 | 4.3e-04   db 3.7e-01 | 5.8e-05        color_branch.0  dW 3.7e-01 | 5.2e-04   db 3.1e-02 | 8.7e-06
    block1.2  dW 6.7e-01 | 3.1e-04   db 3.0e-01 | 6.5e-05        color_branch.2  dW 4.4e-01 | 4.1e-04   db 3.2e-02 | 1.6e-05
    block3.0  dW 7.7e-01 | 3.7e-04   db 4.4e-01 | 1.2e-04        color_branch.4  dW 3.3e-01 | 4.5e-04   db 1.2e-05 | 1.4e-05
    block3.2  dW 9.3e-01 | 2.8e-04   db 7.2e-01 | 6.7e-05        (row error / the row's own max |f64| on the muted rows: 0.24 .. 0.82)
with every tensor within 9e-5 of its maximum.  With the scales the muted rows are at 2.4e-04 .. 5.1e-04 (dW) and 1.2e-05 .. 8.1e-05 (db)."""
import pytest
import torch

import gpu_util
import wgrad_rows_case as WR
from emu_util import emu_backend

_refs = {}


def _ref(k):
    if k not in _refs:
        _refs[k] = WR.Reference("emu", k)
        _refs[k].check_conditions()
    return _refs[k]


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("k", [0, 4])
def test_emulated_weight_gradient_rows_muted_units(k):
    WR.run(_ref(k), gpu_util.hip_render, 8, 1)


@pytest.mark.parametrize("k", [0, 4])
def test_the_one_plane_format_meets_its_own_bar(k):
    """the bar of the one-plane mode, tested on the format it is derived from (exact sums, no exponent limit)"""
    _ref(k).check_ideal()

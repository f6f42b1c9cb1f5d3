"""Host-emulator twin of tests/test_gpu_gradient_range.py (tests/range_case.py): the aggregator backward on rays whose probe is 10^-k of the
others', gradients of the points only those rays touch against float64, relative to THEIR OWN largest gradient.  The emulator shares the
formats, scales and quantisation code with the device and differs in accumulation order only; an emulated backward of this size takes
15-25 s, hence k in {0, 5}: e4m3 cross terms (shipped) at both, f16 cross terms at k = 5."""
import pytest
import torch

import gpu_util
import range_case as RC
from emu_util import emu_backend


@pytest.fixture(scope="module")
def ref():
    r = RC.Reference("emu")
    r.check_conditions()
    return r


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


def test_emulated_down_weighted_rays_e4m3_cross_terms(ref):
    RC.run_arithmetic(ref, gpu_util.hip_render, 8, (0, 5), extras=False)


def test_emulated_down_weighted_rays_f16_cross_terms(ref):
    RC.run_arithmetic(ref, gpu_util.hip_render, 16, (5,), extras=False)

"""tests/query_case.py on the HOST-EMULATED kernels (tools/emu): the CPU-suite twin of test_query_cases_* in tests/test_gpu_query.py.  An axis
swapped in the dilation loop, the brick addressing or the occupancy index, a P cap that keeps other points than the first P, a `<` for a `<=`
in the insertion fails here, before any GPU time is spent.  What only the device can show -- how grid.hip and query.hip are compiled there:
division, contraction -- stays with the -m gpu tests: the emulator divides and multiplies with the host's arithmetic."""
import pytest
import torch

import query_case as QC
from emu_util import emu_backend


@pytest.fixture(autouse=True)
def _emu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    with emu_backend():
        yield


@pytest.mark.parametrize("name", QC.NAMES)
def test_emulated_query_cases_native_op_bit_exact(name):
    fig = QC.conditions(name)
    print(name, fig)
    QC.check(name, "cpu")


@pytest.mark.parametrize("name", [n for n in QC.NAMES if n[0] in "AB"])
def test_emulated_query_cases_fused_ray_generation(name):
    QC.conditions(name)
    QC.check_dense(name, "cpu")

"""Host-emulator twin of tests/test_gpu_raymarch.py (tests/raymarch_case.py): the real k_raymarch_forward / k_raymarch_backward, built for
x86, against float64 per slot and per ray, with the same cases, bars and bit conditions.  The emulator's expf is the host's libm; the order of
every wave scan and sum is the device's."""
import pytest
import torch

import raymarch_case as RC
from emu_util import emu_backend
from oracle import pyref

_runs = {}


@pytest.fixture(autouse=True)
def _emu():
    with emu_backend():
        yield


def _run(case):
    if case not in _runs:
        _runs[case] = RC.hip_case(RC.reference(case), "cpu")
    return _runs[case]


def test_reference_formula_is_pyref_ray_march():
    RC.check_pinned_to_pyref(pyref)


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_emulated_forward_per_slot_against_float64(case):
    RC.check_forward(RC.reference(case), _run(case)[0])


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_emulated_backward_per_ray_against_float64(case):
    RC.check_backward(RC.reference(case), _run(case)[1])


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_emulated_exact_conditions(case):
    RC.check_exact(RC.reference(case), *_run(case))


@pytest.mark.parametrize("SR", (1, 65, 130))
def test_emulated_gradient_scales_by_exact_powers_of_two(SR):
    RC.check_scaling(RC.reference(("thin", SR, "white")), "cpu")


@pytest.mark.parametrize("case", [("thin", 65, "white"), ("opaque", 65, "white")], ids=RC.case_id)
def test_emulated_ray_does_not_depend_on_the_others_or_on_memory_around(case):
    ref = RC.reference(case)
    out, grad = _run(case)
    for r in (0, ref.rows["surface"][-1], RC.R - 1):
        RC.check_ray_alone(ref, out, grad, "cpu", r)
    RC.check_guarded_memory(ref, out, grad, "cpu")


def test_emulated_return_codes():
    RC.check_return_codes("cpu")

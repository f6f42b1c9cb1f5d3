"""The ray march alone on the device (tests/raymarch_case.py): pointnerf_amd.diff_ray_marching.ray_march on inputs built for it -- thin,
mixed and opaque rays of 1, 63, 64, 65, 130 and 160 slots, hand-built empty / single-slot / hard-surface / zero-distance rays -- against
float64.  Forward: every output per slot within the project's forward bar.  Backward: per ray, E = max_s |d - d64| / max_s |d64| for d sigma
and for d rgb; the kernel's median, 95th percentile and maximum of E are at most 2 x the fp32 oracle's (opaque: on the rays where the oracle
itself is within 1e-5, E <= 2e-5 and the median at most 2 x the oracle's).  Bit conditions: invalid slots, empty and zero-gradient rays,
power-of-two gradient scales, two calls, a ray alone, guarded memory around every array; the return codes of the two entry points."""
import pytest
import torch

import raymarch_case as RC
from gpu_util import DEV
from oracle import pyref

pytestmark = pytest.mark.gpu
_runs = {}


def _run(case):
    """one forward + backward of a case on the device, shared by the tests of the case"""
    if case not in _runs:
        _runs[case] = RC.hip_case(RC.reference(case), DEV)
    return _runs[case]


def test_reference_formula_is_pyref_ray_march():
    RC.check_pinned_to_pyref(pyref)


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_forward_per_slot_against_float64(case):
    RC.check_forward(RC.reference(case), _run(case)[0])


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_backward_per_ray_against_float64(case):
    RC.check_backward(RC.reference(case), _run(case)[1])


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_exact_conditions_and_two_calls(case):
    ref = RC.reference(case)
    out, grad = _run(case)
    RC.check_exact(ref, out, grad)
    out2, grad2 = RC.hip_case(ref, DEV)
    for k in RC.FORWARD_KEYS:
        assert torch.equal(out2[k], out[k]), (case, k, "two calls, different bits")
    assert torch.equal(grad2, grad), (case, "two calls, different gradient bits")


@pytest.mark.parametrize("SR", RC.SRS)
def test_gradient_scales_by_exact_powers_of_two(SR):
    RC.check_scaling(RC.reference(("thin", SR, "white")), DEV)


@pytest.mark.parametrize("case", [("thin", 65, "white"), ("opaque", 65, "white"), ("thin", 130, "white"), ("opaque", 160, "white")], ids=RC.case_id)
def test_ray_does_not_depend_on_the_others_or_on_memory_around(case):
    ref = RC.reference(case)
    out, grad = _run(case)
    for r in (0, ref.rows["surface"][-1], RC.R - 1):
        RC.check_ray_alone(ref, out, grad, DEV, r)
    RC.check_guarded_memory(ref, out, grad, DEV)


def test_return_codes():
    RC.check_return_codes(DEV)

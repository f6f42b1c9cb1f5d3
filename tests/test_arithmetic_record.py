"""The process-wide arithmetic settings (csrc/aggregate.hip: PnArith) are one record with one read entry point, pnerf_get_arithmetic:
{inference products, weight-gradient planes, cross-term bits, cross-term mask as stored}.  The four setters return the previous value and
refuse a bad argument without touching the record; ops.cross_terms_state() / ops.frames_table() read and never write.  Host code only: the
emulator library, and child processes that load nothing else (no GPU is opened)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from emu_util import emu_backend, emu_lib

CHILD = ("import ctypes, sys; h = ctypes.CDLL(sys.argv[1]); out = (ctypes.c_int32 * 4)(); "
         "assert h.pnerf_get_arithmetic(out) == 0; print(*out)")


def _get(h):
    out = (ctypes.c_int32 * 4)()
    assert h.pnerf_get_arithmetic(out) == 0
    return tuple(out)


@pytest.mark.parametrize("env_mask,expect", [(None, (3, 1, 8, 4)), ("3", (3, 1, 8, 3)), ("11", (3, 1, 8, 3))])
def test_defaults_in_a_fresh_process(env_mask, expect):
    env = {k: v for k, v in os.environ.items() if k != "PNERF_MIX_MASK"}
    if env_mask is not None:
        env["PNERF_MIX_MASK"] = env_mask
    r = subprocess.run([sys.executable, "-c", CHILD, emu_lib()._name], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr
    assert tuple(int(v) for v in r.stdout.split()) == expect


def test_null_pointer_is_refused():
    assert emu_lib().pnerf_get_arithmetic(None) < 0


# (setter, index in the record, its valid values, bad arguments)
SETTERS = [("pnerf_set_inference_products", 0, (2, 3), (1, 4, 0, -1)),
           ("pnerf_set_wgrad_planes", 1, (1, 2), (0, 3, -1)),
           ("pnerf_set_cross_terms", 2, (8, 16), (0, 4, 32, -8)),
           ("pnerf_set_cross_terms_where", 3, (0, 1, 2, 3, 4, 5, 6, 7), (-1, 8, 255))]


@pytest.mark.parametrize("name,idx,good,bad", SETTERS)
def test_setter_shows_in_the_getter_and_returns_the_old_value(name, idx, good, bad):
    h = emu_lib()
    fn = getattr(h, name)
    start = _get(h)
    try:
        for v in good + good[::-1]:
            before = _get(h)
            assert fn(v) == before[idx]
            after = _get(h)
            assert after[idx] == v and after[:idx] + after[idx + 1:] == before[:idx] + before[idx + 1:]
            for b in bad:
                assert fn(b) < 0 and _get(h) == after
    finally:
        fn(start[idx])
    assert _get(h) == start


class _NoSetters:
    """the library handle with every pnerf_set_* taken away"""
    def __init__(self, h):
        self._h = h

    def __getattr__(self, name):
        assert not name.startswith("pnerf_set_"), "a reader wrote: " + name
        return getattr(self._h, name)


def test_python_readers_do_not_write():
    from pointnerf_amd import _lib as L, ops
    frames = torch.eye(3).repeat(5, 1, 1)
    with emu_backend() as h:
        start = _get(h)
        try:
            for bits, where in ((8, 4), (8, 6), (16, 5)):
                ops.set_cross_terms(bits, where=where)
                record = _get(h)
                assert ops.arithmetic() == record == (start[0], start[1], bits, where)
                L._lib = _NoSetters(h)
                try:
                    assert ops.cross_terms_state() == (bits, where if bits == 8 else 0)
                    assert ops.frames_table(frames, 5).shape == (5, 9)
                finally:
                    L._lib = h
                assert _get(h) == record
        finally:
            ops.set_cross_terms(start[2], where=start[3])
        assert _get(h) == start


def test_set_wgrad_planes_still_drops_the_cached_capacities():
    from pointnerf_amd import ops
    with emu_backend():
        ops.ARENA._cap_cache = {"stale": 1}
        old = ops.set_wgrad_planes(2)
        try:
            assert ops.ARENA._cap_cache == {} and ops.arithmetic()[1] == 2
        finally:
            ops.set_wgrad_planes(old)

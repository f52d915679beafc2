"""CPU: dml_coalescer_set_key_range and dml_diag_coalesce_order refuse before any HIP call. A zeroed
buffer stands for the context: a refusal leaves it so; to the diagnostic it has completed no call."""
import ctypes as C

import pytest

from distml_amd import _lib

E, U = _lib.DML_E_INVALID_ARG, _lib.DML_E_UNSUPPORTED
BIG = 1 << 32
ctx = lambda: C.create_string_buffer(512)  # noqa: E731


@pytest.mark.parametrize("first,last,want", [(5, 4, E), (0, -1, E), (0, BIG + 1, U), (-BIG, 1, U),
                                             (-(1 << 63), (1 << 63) - 1, U)])
def test_setter_refuses(first, last, want):
    c = ctx()
    assert _lib.load().dml_coalescer_set_key_range(C.addressof(c), first, last) == want
    assert bytes(c.raw) == b"\0" * 512  # the context is unchanged
    assert _lib.load().dml_coalescer_set_key_range(None, 0, 10) == E


@pytest.mark.parametrize("first,last", [(0, BIG), (-1000, -800), ((1 << 63) - 201, (1 << 63) - 1)])
def test_setter_accepts_and_clears(first, last):
    c = ctx()
    L = _lib.load()
    assert L.dml_coalescer_set_key_range(C.addressof(c), first, last) == 0
    assert bytes(c.raw) != b"\0" * 512
    assert L.dml_coalescer_set_key_range(C.addressof(c), first, first) == 0  # first == last clears it
    assert bytes(c.raw) == b"\0" * 512


def test_diagnostic_refuses():
    c, out = ctx(), (C.c_int32 * 3)(7, 7, 7)
    L = _lib.load()
    assert L.dml_diag_coalesce_order(None, out) == E
    assert L.dml_diag_coalesce_order(C.addressof(c), None) == E
    assert L.dml_diag_coalesce_order(C.addressof(c), out) == E  # before any call
    assert "no completed" in _lib.last_error() and list(out) == [7, 7, 7]


"""CPU: dml_compact_rows_expand_device's refusals, which the header promises before any HIP call (the
pointers are made-up addresses no kernel may ever see); n == 0 and m == 0 are DML_OK with nothing launched."""
import pytest

from distml_amd import _lib

M, ENT, COLS, N = 7, 40, 5, 9
PTR, EC, EV, INV, OUT = (0x10000000 + i * 0x100000 for i in range(5))
CASES = {"m-negative": dict(m=-1), "n-negative": dict(n=-1), "entries-negative": dict(ent=-1), "cols-0": dict(cols=0),
         "cols-negative": dict(cols=-3), "m-2^31": dict(m=1 << 31), "n-2^31": dict(n=1 << 31),
         "null-inverse-n-not-m": dict(inv=0), "ptr-null": dict(ptr=0), "ecol-null": dict(ec=0), "eval-null": dict(ev=0),
         "plane-null": dict(out=0), "ptr-misaligned": dict(ptr=PTR + 2), "ecol-misaligned": dict(ec=EC + 1),
         "eval-misaligned": dict(ev=EV + 3), "inverse-misaligned": dict(inv=INV + 2), "plane-misaligned": dict(out=OUT + 2),
         "plane-over-ptr": dict(out=PTR + 4 * M), "plane-over-ecol": dict(out=EC - 4 * (N * COLS - 1)),
         "plane-over-eval": dict(out=EV + 4 * (ENT - 1)), "plane-over-inverse": dict(out=INV + 4 * (N - 1)),
         "plane-bytes-overflow": dict(n=(1 << 31) - 1, cols=(1 << 31) - 1)}


def call(**over):
    a = {**dict(ptr=PTR, ec=EC, ev=EV, m=M, ent=ENT, cols=COLS, inv=INV, n=N, out=OUT), **over}
    return _lib.load().dml_compact_rows_expand_device(a["ptr"] or None, a["ec"] or None, a["ev"] or None, a["m"], a["ent"],
                                                      a["cols"], a["inv"] or None, a["n"], a["out"] or None, None)


@pytest.mark.parametrize("what", CASES)
def test_refusal(what):
    assert call(**CASES[what]) == _lib.DML_E_INVALID_ARG and _lib.last_error()


def test_nothing_to_expand():
    assert call(n=0) == call(n=0, out=0, inv=0, m=0, ptr=0) == call(m=0, ptr=0, ent=0, ec=0, ev=0) == 0

"""CPU: dml_coalesce_elems_device's refusals, which the header promises before any HIP call and
before the context is dereferenced (a dummy non-null handle stands for it), leave *out_rows and
*out_len as they were; n == 0 is DML_OK with both 0."""
import ctypes as C

import pytest

from distml_amd import DataDesc, _lib

E, U = _lib.DML_E_INVALID_ARG, _lib.DML_E_UNSUPPORTED
N, COLS = 9, 5
K, CP, VP, OUT, KO, IO = (0x10000000 + i * 0x100000 for i in range(6))
GOOD = dict(fmt=DataDesc(1, 0, 0, False, True, False), cols=COLS, flags=0, keys=K, n=N, per=2, cp=CP, vp=VP, form=1,
            out=OUT, cap=1 << 16, ko=KO, io=IO)

CASES = [("f32", dict(fmt=DataDesc(1, 0, 1, False, True, False)), U),
         ("f64", dict(fmt=DataDesc(1, 1, 3, False, True, False)), U),
         ("adagrad", dict(fmt=DataDesc(1, 0, 1, False, True, True)), U),
         ("array", dict(fmt=DataDesc(0, 0, 0)), U),
         ("sparse-column", dict(fmt=DataDesc(1, 0, 0, False, False, False)), U),
         ("per-0", dict(per=0), E), ("per-17", dict(per=17), E), ("form-2", dict(form=2), E),
         ("flag", dict(flags=0x40000000), E), ("n-negative", dict(n=-1), E),
         ("out-misaligned", dict(out=OUT + 2), E), ("cols-misaligned", dict(cp=CP + 1), E),
         ("keys-misaligned", dict(keys=K + 4), E), ("vals-null", dict(vp=0), E), ("out-null", dict(out=0), E),
         ("rows-without-keys-out", dict(form=0, ko=0), E),
         ("out-over-cols", dict(out=CP + 4 * (2 * N - 1)), E), ("inverse-over-vals", dict(io=VP - 4 * (N - 1)), E),
         ("keys-out-over-keys", dict(ko=K + 8 * (N - 1)), E)]


def call(**over):
    a = {**GOOD, **over}
    dummy = C.create_string_buffer(256)
    m, ln = C.c_int64(-7), C.c_int64(-7)
    rc = _lib.load().dml_coalesce_elems_device(C.addressof(dummy), C.byref(a["fmt"].to_c()), a["cols"], a["flags"],
                                               a["keys"], a["n"], a["per"], a["cp"], a["vp"], a["form"], a["out"],
                                               a["cap"], a["ko"], a["io"], C.byref(m), C.byref(ln), None)
    assert bytes(dummy.raw) == b"\0" * 256  # the handle was not written
    return rc, m.value, ln.value


@pytest.mark.parametrize("what,over,want", CASES, ids=[c[0] for c in CASES])
def test_refusal(what, over, want):
    assert call(**over) == (want, -7, -7)
    if what == "array":
        assert "dml_coalesce_device" in _lib.last_error()


@pytest.mark.parametrize("form", [0, 1])
def test_empty_list(form):
    assert call(n=0, form=form) == (0, 0, 0)
    assert call(n=0, form=form, keys=0, cp=0, vp=0, out=0, ko=0, io=0) == (0, 0, 0)

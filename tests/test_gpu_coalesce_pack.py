"""dml_coalesce_pack_device (Coalescer.run_packed), byte for byte against the host encoders'
records of ce.coalesce(keys, v); arenas between canaries at leads of 4 and 12 mod 16."""
import ctypes as C

import numpy as np
import pytest

import coalesce_expect as ce
import geom
from test_gpu_coalesce import _gpu, co, desc, same, tiles  # noqa: F401  (_gpu: the module's GPU gate)
from test_gpu_coalesce_long import LAYOUTS, NEVER, edge_keys, lo, routed, sizes  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
REF = 1  # DML_FLAG_FLOAT_ARRAY_REF_STRIDE


def check(co, fmt, cols, keys, v, lead=4, flags=0, extra=0, outs=True, stream=None, what=()):
    """One run_packed against the host encode and the model, canaries and inputs intact."""
    from distml_amd import DeviceKeys, encode_array_push, encode_matrix_push
    n, (uk, inv, sums) = len(keys), ce.coalesce(keys, v)
    rec = (encode_matrix_push(uk, sums, fmt.keyType, fmt.valueType) if fmt.dataType == 1 else
           encode_array_push(uk, sums.reshape(-1), fmt.keyType, fmt.valueType, 8 if flags & REF else None))
    ka, va = geom.pack([keys.tobytes()], lead & 8), geom.pack([v.tobytes()], 16 - lead)
    ro = geom.OutArena(len(rec) + extra, lead).upload()
    io = geom.OutArena(n * 4, 16 - lead).upload() if outs else None
    ko = geom.OutArena(len(uk) * 8, 8 - (lead & 8)).upload() if outs else None
    got = co.run_packed(fmt, cols, DeviceKeys(ka.ptrs[0], n), va.ptrs[0], ro.ptr, len(rec) + extra,
                        io.ptr if outs else None, ko.ptr if outs else None, stream=stream, flags=flags)
    torch.cuda.synchronize()
    assert got == (len(uk), len(rec)), (what, got)
    same(ro.read()[:len(rec)], rec, ("records",) + tuple(what))
    ro.untouched([(0, len(rec))])
    if outs:
        same(io.read(), inv.tobytes(), ("inverse",) + tuple(what))
        same(ko.read(), uk.tobytes(), ("keys",) + tuple(what))
    ka.check()
    va.check()
    return rec


@pytest.mark.parametrize("i", range(len(LAYOUTS)), ids=[l[0] for l in LAYOUTS])
def test_layouts_both_paths(lo, i):
    """The long path's 11 layouts with the threshold at T: one list holds walk and long segments."""
    tag, dt, kt, vt, cols, ada, first = LAYOUTS[i]
    rowcols = cols if dt == 1 else 1
    keys = edge_keys(first, rowcols * ce.VDT[vt]().itemsize < 16, seed=i)
    v = ce.values(vt, len(keys), rowcols, seed=i)
    check(lo, desc(dt, kt, vt, ada), cols, keys, v, (4, 12)[i % 2], extra=8 * (i % 3), outs=i % 4 != 3, what=(tag,))
    assert lo.route() == routed(keys, sizes()[0]), tag


@pytest.mark.parametrize("pat", ["skewed", "equal", "asc"])
@pytest.mark.parametrize("dt,cols,flags", [(1, 50, 0), (1, 257, 0), (0, 1, 0), (0, 1, REF)])
def test_walk_edges(co, dt, cols, flags, pat):
    """Segments around DML_COALESCE_DEPTH / _BATCH, one key, all distinct; the array with and without its pad."""
    _, batch, depth = tiles()
    keys = ce.patterns(geom.NEG32, 300, depth, batch, seed=cols)[pat]
    v = ce.values(1, len(keys), cols, seed=3)
    check(co, desc(dt, 0, 1), cols, keys, v, 12 if flags else 4, flags=flags, extra=16, what=(pat, cols, flags))
    assert co.route() == (0, 0)


@pytest.mark.parametrize("vt", [1, 3, 0], ids=["f32", "f64", "i32"])
def test_special_values(co, vt):
    """Negative quiet NaN, +0.0 from a lone -0.0, ties-to-even order, int32 wrap, inside records."""
    keys, v = ce.special_case(vt)
    check(co, desc(1, 1, vt), 4, keys, v, 4, what=("specials",))
    check(co, desc(0, 0, vt), 1, keys, np.ascontiguousarray(v[:, :1]), 12, what=("specials", "array"))


def test_same_bytes_as_two_calls(lo):
    """run + pack_push_device, then run_packed at never, at T and twice on a stream: the same bytes."""
    from distml_amd import DeviceKeys, pack_push_device
    fmt, cols, T = desc(1, 1, 1), 200, sizes()[0]
    keys = edge_keys(geom.BIG33, False, seed=7)
    v = ce.values(1, len(keys), cols, seed=7)
    n, m, R = len(keys), len(np.unique(keys)), 8 + 4 * cols
    ka, va = geom.pack([keys.tobytes()], 0), geom.pack([v.tobytes()], 4)
    ko, so, po = geom.OutArena(m * 8, 8).upload(), geom.OutArena(m * cols * 4, 4).upload(), geom.OutArena(m * R, 12).upload()
    assert lo.run(fmt, cols, DeviceKeys(ka.ptrs[0], n), va.ptrs[0], ko.ptr, so.ptr, None, m) == m
    assert pack_push_device(fmt, cols, DeviceKeys(ko.ptr, m), so.ptr, m, po.ptr, m * R) == m * R
    st = torch.cuda.Stream().cuda_stream
    for thr, stream in ((NEVER, None), (T, None), (T, st), (T, st)):  # ends at T, the fixture's threshold
        lo.set_long_min(thr)
        assert check(lo, fmt, cols, keys, v, 12, stream=stream, what=(thr, stream)) == po.read().tobytes()


def test_refusals(co):
    """Each argument error (argument index, value, status), the first also on a stream: outs untouched.
    cap = m x R - 4: DML_E_CAPACITY with the needed sizes. Every output is still canary; then the call works."""
    from distml_amd import DataDesc, _lib
    E, U, BD = _lib.DML_E_INVALID_ARG, _lib.DML_E_UNSUPPORTED, _lib.DML_E_BAD_DESC
    n, cols, fmt, cap = 9, 5, desc(1, 1, 1), 9 * (8 + 4 * 5)
    keys, v = geom.BIG33 + np.arange(n, dtype=np.int64), ce.values(1, n, cols)
    ka, va = geom.pack([keys.tobytes()], 8), geom.pack([v.tobytes()], 4)
    ko, ro, io = geom.OutArena(n * 8, 8).upload(), geom.OutArena(cap, 12).upload(), geom.OutArena(n * 4, 4).upload()
    K, V, RO = ka.ptrs[0], va.ptrs[0], ro.ptr
    good = [fmt, cols, 0, K, n, V, RO, cap, ko.ptr, io.ptr]
    # misaligned records; records over keys, values, inverse; null values; unknown flag; sparse column; bad desc
    cases = [(6, RO + 2, E), (6, K + 8 * n - 4, E), (6, V - cap + 4, E), (6, io.ptr + 4 * n - 4, E), (5, 0, E),
             (2, 0x40000000, E), (0, DataDesc(1, 1, 1, False, False, False), U), (0, DataDesc(1, 1, 2, False, True, False), BD),
             (7, cap - 4, _lib.DML_E_CAPACITY)]
    for stream in (None, torch.cuda.Stream().cuda_stream):
        for at, value, want in cases if stream is None else cases[:1]:
            a, m, ln = good[:at] + [value] + good[at + 1:], C.c_int64(-7), C.c_int64(-7)
            rc = _lib.load().dml_coalesce_pack_device(co._h, C.byref(a[0].to_c()), *a[1:], C.byref(m), C.byref(ln), stream)
            assert (rc, m.value, ln.value) == ((want, n, cap) if at == 7 else (want, -7, -7)), (at, value)
    for a in (ko, ro, io):
        a.read()
        a.untouched([])
    check(co, fmt, cols, keys, v, 12, what=("after the refusals",))

"""CPU: the numpy model of dml_coalesce_device (tests/coalesce_expect.py) is the reference's
result, it tells summation orders apart, and the call's argument refusals, which the header
promises before any HIP call, hold on a machine without a GPU."""
import ctypes as C

import numpy as np
import pytest

import coalesce_expect as ce
import codec_cases as cc
import fetch_cases as fc
import geom

ROWS, NOCC = 97, 1500

# (tag, data type, key type, value type, cols, first key)
ANCHORS = [("f32", 1, 0, 1, 5, geom.NEG32), ("f64", 1, 1, 3, 5, geom.BIG33), ("af32", 0, 1, 1, 1, geom.BIG33),
           ("af64", 0, 0, 3, 1, 1000), ("i32", 1, 0, 0, 5, 1000), ("ai32", 0, 1, 0, 1, geom.STRADDLE)]


def occurrences(case, seed=3):
    """NOCC occurrences over the case's ROWS rows: magnitudes over 1e-3 .. 1e3 and one -0.0
    (floats); int32 values >= 0, so every prefix sum is a counter the reference accepts."""
    rng = np.random.default_rng(seed)
    keys = case["first"] + rng.integers(0, ROWS, size=NOCC).astype(np.int64)
    if case["vt"] == 0:
        v = rng.integers(0, 1000, size=(NOCC, case["cols"])).astype(np.int32)
    else:
        v = ce.values(case["vt"], NOCC, case["cols"], seed + 1)
        v[7, 0] = -0.0
    return keys, v


def push_bytes(case, keys, v):
    from distml_amd import encode_array_push, encode_matrix_push
    if case["dt"] == 1:
        return encode_matrix_push(keys, v, case["kt"], case["vt"])
    return encode_array_push(keys, v.ravel(), case["kt"], case["vt"])


@pytest.mark.parametrize("a", ANCHORS, ids=lambda a: a[0])
def test_model_is_the_oracle(oracle, a):
    """Oracle anchor. A zero OracleStore given ONE push of the occurrences as records in list
    order, then a fetch of the sorted unique keys, yields exactly the model's keys and value
    bytes (FloatMatrixStore.java:200-222: localData[row][c] += value, record after record)."""
    case = fc._case(*a[:5], ROWS, a[5])
    keys, v = occurrences(case)
    o = oracle.OracleStore(case["dt"], case["kt"], case["vt"], case["first"], case["first"] + ROWS - 1, case["cols"])
    assert not o.data.any()
    assert o.push(push_bytes(case, keys, v)) == 0
    uk, inv, sums = ce.coalesce(keys, v)
    assert len(uk) == ROWS and (uk[inv] == keys).all() and (np.diff(uk) > 0).all()
    fk, fv, _ = cc.unpack_expected(case, o.fetch(uk))
    assert fk.tobytes() == uk.tobytes()
    assert fv.tobytes() == sums.tobytes()
    if case["vt"] != 0:
        assert np.isfinite(sums).all()


@pytest.mark.parametrize("vt", [1, 3], ids=["f32", "f64"])
def test_model_tells_orders_apart(vt):
    """Yardstick. The same occurrences in reversed list order change a large share of the value
    words (measured on this input: 70 % of the f32 words, 67 % of the f64 ones), so a kernel
    that summed in another order would not pass a byte comparison with the model."""
    case = fc._case("m", 1, 0, vt, 5, ROWS, 1000)
    keys, v = occurrences(case)
    uk, _, fwd = ce.coalesce(keys, v)
    uk2, _, rev = ce.coalesce(keys[::-1], v[::-1])
    assert uk.tobytes() == uk2.tobytes()
    share = float((fwd != rev).mean())
    print("share of value words that differ:", share)
    assert share > 0.25


def test_model_edges():
    """The model itself on the contract's special values: a lone -0.0 comes out +0.0, a
    signalling NaN quiet, int32 wraps, order decides a ties-to-even triple, keys ascend as
    signed values."""
    k, v = ce.special_case(1)
    uk, inv, s = ce.coalesce(k, v)
    raw = s.view(np.uint32)
    assert raw[0, 0] == 0 and raw[0, 1] == 0 and raw[0, 3] == 0           # lone -0.0 -> +0.0
    assert raw[1, 0] == 0 and raw[2, 3] == 0                               # -0.0 + -0.0 from +0.0
    assert raw[3, 1] == 0x7FC12345 and raw[3, 3] == 0x7FE00001             # payload kept; sNaN quiet
    assert np.isnan(s[4, 0]) and np.isnan(s[4, 1]) and s[4, 2] == np.inf   # +Inf then -Inf
    assert s[6, 0] == 2.0 ** 24 and s[7, 0] == 2.0 ** 24 + 2               # ties to even: order decides
    k, v = ce.special_case(0)
    _, _, s = ce.coalesce(k, v)
    assert s[0, 0] == -(1 << 31) and s[1, 0] == -(1 << 30) - 1 and s[2, 0] == -(1 << 31)
    uk, inv, _ = ce.coalesce(np.array([5, ce.INT64_MAX, -1, ce.INT64_MIN, 5], np.int64))
    assert uk.tolist() == [ce.INT64_MIN, -1, 5, ce.INT64_MAX] and inv.tolist() == [2, 3, 1, 0, 2]


def test_refusals_need_no_device():
    """Every DML_E_INVALID_ARG / _BAD_DESC / _UNSUPPORTED case returns its code with *out_rows
    untouched, and n == 0 is DML_OK with 0, before any HIP call: the context is a dummy
    non-null handle, which the header's "checked before `c` is dereferenced" allows, so this
    runs without a GPU. (tests/test_gpu_coalesce.py repeats the table with a real context and
    live arenas, and covers DML_E_CAPACITY, which needs the device.)"""
    from distml_amd import DataDesc, _lib
    L = _lib.load()
    fmt = DataDesc(1, 1, 1, False, True, False)
    dummy = C.create_string_buffer(256)
    c = C.addressof(dummy)
    n, cols = 9, 5
    K, V, KO, VO, IO = (0x10000000 + i * 0x100000 for i in range(5))
    for what, args, want in ce.refusal_cases(K, V, KO, VO, IO, n, cols):
        assert ce.raw_call(L, c, *args) == (want, -7), what
    assert ce.raw_call(L, 0, fmt, cols, K, n, V, KO, VO, IO, n) == (_lib.DML_E_INVALID_ARG, -7)
    assert ce.raw_call(L, c, fmt, cols, K, n, V, KO, VO, IO, n, out_rows=False)[0] == _lib.DML_E_INVALID_ARG
    assert ce.raw_call(L, c, fmt, cols, K, 0, V, KO, VO, IO, n) == (0, 0)
    assert ce.raw_call(L, c, fmt, cols, 0, 0, 0, 0, 0, 0, 0) == (0, 0)
    assert ce.raw_call(L, c, DataDesc(0, 0, 0), 0, 0, 0, 0, 0, 0, 0, 0) == (0, 0)
    assert bytes(dummy.raw) == b"\0" * 256  # and the handle was not written either


def test_exported_tile_sizes():
    from distml_amd import _lib
    src = open(geom.__file__.replace("tests/geom.py", "include/distml_ps.h")).read()
    for name in ("DML_COALESCE_BLOCK_KEYS", "DML_COALESCE_BATCH", "DML_COALESCE_DEPTH"):
        assert f"#define {name} {getattr(_lib, name)}\n" in src, name
    assert _lib.DML_COALESCE_BATCH % _lib.DML_COALESCE_DEPTH == 0

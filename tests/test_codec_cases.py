"""CPU: pins tests/codec_cases.py, the yardstick of tests/test_gpu_codec.py. The numpy
expectations tell the layouts apart: unpack-expected inverts pack-expected wherever the
push and the fetch layout coincide, AdaGrad's value and alpha planes differ, FloatArrayStore's
pad is dropped, int32 keys are cut to four bytes by the writer and sign-extended by the
reader; and the library's dml_record_bytes agrees with the table's record sizes."""
import ctypes as C

import numpy as np
import pytest

import codec_cases as cc
import fetch_cases as fc


def test_table_covers_every_store_and_residue():
    stores = {c["store"] for c in cc.CASES}
    assert stores == {"f32", "i32", "f64", "ada", "ai32", "af32", "af32ref", "af64"}
    for tag in ("f32", "i32", "f64", "ada"):
        mine = [c for c in cc.CASES if c["store"] == tag]
        assert {c["cols"] for c in mine} == set(fc.WIDTHS) and {c["kt"] for c in mine} == {0, 1}
        assert {cc.push_record_bytes(c) % 16 for c in mine} == {0, 4, 8, 12}
    firsts = {c["first"] for c in cc.CASES}
    assert any(f > 1 << 32 for f in firsts) and any(f < 0 for f in firsts)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c["id"])
def test_record_bytes_match_the_library(case):
    from distml_amd import DataDesc, record_bytes
    fmt = DataDesc(case["dt"], case["kt"], case["vt"], False, True, case["ada"])
    assert record_bytes(fmt, case["cols"], cc.flags(case)) == (cc.push_record_bytes(case), fc.record_bytes(case))
    assert cc.fetch_dtype(case).itemsize == fc.record_bytes(case)


def test_record_bytes_refusals():
    from distml_amd import DataDesc, _lib
    L = _lib.load()
    p, f = C.c_int64(-1), C.c_int64(-1)
    ok = DataDesc(1, 0, 1, False, True, False).to_c()
    assert L.dml_record_bytes(C.byref(ok), 5, 0, None, None) == 0
    assert L.dml_record_bytes(C.byref(ok), 5, 0, C.byref(p), None) == 0 and p.value == 24
    assert L.dml_record_bytes(C.byref(ok), 5, 0, None, C.byref(f)) == 0 and f.value == 24
    assert L.dml_record_bytes(None, 5, 0, C.byref(p), C.byref(f)) == _lib.DML_E_INVALID_ARG
    assert L.dml_record_bytes(C.byref(ok), 0, 0, C.byref(p), C.byref(f)) == _lib.DML_E_INVALID_ARG
    assert L.dml_record_bytes(C.byref(ok), 5, 0x100, C.byref(p), C.byref(f)) == _lib.DML_E_INVALID_ARG
    sparse = DataDesc(1, 0, 1, False, False, False).to_c()
    assert L.dml_record_bytes(C.byref(sparse), 5, 0, C.byref(p), C.byref(f)) == _lib.DML_E_UNSUPPORTED
    bad = DataDesc(1, 0, 2, False, True, False).to_c()
    assert L.dml_record_bytes(C.byref(bad), 5, 0, C.byref(p), C.byref(f)) == _lib.DML_E_BAD_DESC
    arr = DataDesc(0, 1, 1, False, True, False).to_c()  # arrays ignore cols
    assert L.dml_record_bytes(C.byref(arr), -7, 1, C.byref(p), C.byref(f)) == 0 and (p.value, f.value) == (16, 16)
    assert L.dml_record_bytes(C.byref(arr), 9, 0, C.byref(p), C.byref(f)) == 0 and (p.value, f.value) == (12, 16)
    assert (p.value, f.value) == (12, 16)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c["id"])
def test_expectations_tell_the_layouts_apart(oracle, case):
    _, o = fc.make_oracle(case, oracle)
    keys = fc.key_lists(case)["shuffled"]
    fetched = o.fetch(keys)
    k, v, a = cc.unpack_expected(case, fetched)
    assert k.dtype == np.int64 and k.tolist() == keys.tolist()
    assert v.dtype == fc.VDT[case["vt"]] and v.shape == (len(keys), case["cols"]) and v.flags.c_contiguous
    rows = (keys - case["first"]).astype(np.int64)
    assert v.tobytes() == o.data.reshape(case["rows"], case["cols"])[rows].tobytes()
    if cc.same_layout(case):
        # the fetched bytes are a push: unpack-expected inverts pack-expected
        assert a is None and cc.pack_expected(case, k, v) == fetched
    elif case["ada"]:
        assert a.shape == v.shape and a.tobytes() == o.alpha.reshape(case["rows"], case["cols"])[rows].tobytes()
        assert a.tobytes() != v.tobytes()  # the two planes are told apart
        assert len(fetched) == len(keys) * (cc.key_bytes(case) + 8 * case["cols"])
        assert cc.pack_expected(case, k, v) != fetched  # AdaGrad's push layout is the plain float one
    else:
        # FloatArrayStore: an 8-byte slot on the wire, 4 bytes in the plane: the pad is dropped
        assert case["store"] in ("af32", "af32ref") and a is None
        assert v.nbytes == 4 * len(keys) and len(fetched) == len(keys) * (cc.key_bytes(case) + 8)
        assert not np.frombuffer(fetched, cc.fetch_dtype(case))["pad"].any()
        padded = cc.pack_expected(dict(case, ref_stride=True), k, v)
        assert padded == fetched  # under the ref-stride flag the push has the slot too
        assert cc.pack_expected(dict(case, ref_stride=False), k, v) != fetched


@pytest.mark.parametrize("kt", [0, 1])
def test_key_truncation_and_sign_extension(kt):
    case = fc._case("f32", 1, kt, 1, 3, 10, 0)
    keys = np.array([5, -3, (1 << 31) + 7, (1 << 40) + 11, -(1 << 35) + 2, (1 << 32) - 1], np.int64)
    vals = cc.pack_values(case, len(keys))
    packed = cc.pack_expected(case, keys, vals)
    k, v, _ = cc.unpack_expected(case, packed)
    assert v.tobytes() == vals.tobytes()
    if kt == 1:
        assert k.tolist() == keys.tolist() == cc.wire_key(case, keys).tolist()
    else:
        # the low four bytes, read back as a signed int32
        assert k.tolist() == [5, -3, -(1 << 31) + 7, 11, 2, -1] == cc.wire_key(case, keys).tolist()
        rec = np.frombuffer(packed, np.uint8).reshape(len(keys), 16)
        assert rec[:, :4].tobytes() == (keys & 0xFFFFFFFF).astype("<u4").tobytes()


def test_values_carry_the_special_bit_patterns():
    for case in (fc._case("f32", 1, 0, 1, 5, 10, 0), fc._case("f64", 1, 1, 3, 5, 10, 0), fc._case("i32", 1, 0, 0, 5, 10, 0)):
        sp = fc.specials(case["vt"])
        raw = cc.pack_values(case, 40).view(sp.dtype).reshape(-1)
        assert set(sp.tolist()) <= set(raw.tolist())
    one = cc.pack_values(fc._case("af32", 0, 0, 1, 1, 10, 0), 1)
    assert one.shape == (1, 1) and one.view("<u4")[0, 0] in fc.specials(1).tolist()


def test_edge_counts():
    from distml_amd import _lib
    W, B = _lib.DML_CODEC_WAVE_BYTES, _lib.DML_CODEC_BLOCK_BYTES
    assert (W, B) == (1024, 4096)
    assert cc.push_record_bytes(cc.EDGE_CASE) == 24 and cc.push_record_bytes(cc.EDGE_ARRAY) == 12
    assert fc.edge_counts(W, B) == cc.edge_counts(24, W, B) == [383, 384, 385, 511, 512, 513]
    assert cc.edge_counts(12, W, B) == [767, 768, 769, 1023, 1024, 1025]
    assert cc.edge_counts(20, W, B) == [767, 768, 769, 1023, 1024, 1025]  # EDGE_CASE's values plane: 5 x 4 bytes
    assert cc.edge_counts(8, W, B) == [383, 384, 385, 511, 512, 513]      # EDGE_ARRAY's: one f64

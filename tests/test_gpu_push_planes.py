"""dml_store_push_planes_device: an occurrence plane straight into the shard. Every comparison is byte
equality of the store (values, AdaGrad's alpha and delta, maxDelta's triple, the error state) with the
CPU oracle fed the host encoder's push of host_accumulate(keys, values). The plane sits in geom.Arena
poison at 4 or 12 mod 16 and must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import codec_cases as cc
import fetch_cases as fc
import geom
from test_gpu_worker_coalesce import host_accumulate
from test_gpu_worker_iteration import _gpu, make_store  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 301
F32 = lambda c: fc._case("f32", 1, 0, 1, c, ROWS, geom.NEG32)  # noqa: E731
F64 = lambda c: fc._case("f64", 1, 1, 3, c, ROWS, geom.STRADDLE)  # noqa: E731
ADA = lambda c: fc._case("ada", 1, 1, 1, c, ROWS, geom.BIG33, True)  # noqa: E731
AF32, AF64 = fc._case("af32", 0, 1, 1, 1, ROWS, geom.BIG33), fc._case("af64", 0, 0, 3, 1, ROWS, 1000)
# rows of 12 B (narrow), 16 B, 20 and 200 B (ragged), 1 KiB and 1 KiB + 4; f64: 8 B, 16 B, 1 KiB + 8; arrays; AdaGrad
SHAPES = [F32(c) for c in (3, 4, 5, 50, 256, 257)] + [F64(c) for c in (1, 2, 129)] + [AF32, AF64] + [ADA(c) for c in (3, 5, 200)]


def pair(case, oracle, init=None, seed=5):
    """(store, oracle store) with the same normal values; rows of -0.0 are the caller's to seed."""
    if init is None:
        init = np.random.default_rng(seed).standard_normal((ROWS, case["cols"])).astype(fc.VDT[case["vt"]])
    o = oracle.OracleStore(case["dt"], case["kt"], case["vt"], case["first"], case["first"] + ROWS - 1, case["cols"], 1,
                           int(case["ada"]), 0)
    case["ada"] and o.set_alpha(*fc.ADA)
    o.data[:] = init
    return make_store(case, init), o


def err(e):
    """(code, key, col); key and col mean something only beside a code."""
    return e if e[0] else (0, 0, -1)


def state(s, case):
    md = s.maxDelta() if case["ada"] else (0.0, 0, 0)
    return ([s.values().tobytes()] + [x.tobytes() for x in (s.adagrad_state() if case["ada"] else ())] +
            [np.float32(md[0]).tobytes(), md[1:], err(s.error_state())])


def ostate(o, case):
    md = o.max_delta() if case["ada"] else (0.0, 0, 0)
    return ([o.data.tobytes()] + ([o.alpha.tobytes(), o.delta.tobytes()] if case["ada"] else []) +
            [np.float32(md[0]).tobytes(), md[1:], err(o.error())])


def push(s, co, keys, vals, lead=4, stream=None):
    """One plane push; returns what must stay alive until the apply stream has passed it."""
    from distml_amd import DeviceKeys
    dk = torch.from_numpy(np.ascontiguousarray(keys, np.int64).copy()).cuda()
    arena = geom.pack([vals.tobytes()], lead)  # synchronises
    s.handlePushPlanesDevice(s.format, co, DeviceKeys(dk.data_ptr(), len(keys)), arena.ptrs[0], stream=stream)
    return dk, arena


def host_push(o, case, keys, vals):
    return o.push(cc.pack_expected(case, *host_accumulate(keys, vals)))


def draw(rng, case, n, pool=None):
    """n occurrences of about n / 3 keys in arbitrary order, and their rows."""
    pool = rng.permutation(ROWS)[:max(1, n // 3)] if pool is None else pool
    keys = case["first"] + pool[rng.integers(0, len(pool), size=n)].astype(np.int64)
    return keys, (rng.standard_normal((n, case["cols"])) * 0.7).astype(fc.VDT[case["vt"]])


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: c["id"])
def test_bytes(case, oracle):
    """n = 1, 63, 65 and 900 in sequence on one store; the plane at 4 and 12 mod 16; rows no call lists
    hold -0.0 in their first column and keep it."""
    from distml_amd import Coalescer
    rng = np.random.default_rng(case["cols"] + len(case["id"]))
    pool = rng.permutation(ROWS)
    init = rng.standard_normal((ROWS, case["cols"])).astype(fc.VDT[case["vt"]])
    init[pool[300:], 0] = -0.0
    (s, o), co = pair(case, oracle, init), Coalescer(0)
    try:
        for i, n in enumerate((1, 63, 65, 900)):
            keys, vals = draw(rng, case, n, pool[:max(1, n // 3)])
            _, arena = push(s, co, keys, vals, lead=(4, 12)[i % 2])
            assert host_push(o, case, keys, vals) == 0
            assert state(s, case) == ostate(o, case), n
            arena.check()
        assert np.signbit(s.values()[pool[300:], 0]).all()
    finally:
        co.close(), s.close()


@pytest.mark.parametrize("case", [F32(257), F32(3), ADA(200), ADA(3)], ids=lambda c: c["id"])
def test_long_route(case, oracle):
    """long_min = 4 and one key with 300 occurrences (two tiles of 128 and a remainder): the bytes of
    the same call with the long path off, and the oracle's."""
    from distml_amd import Coalescer
    rng = np.random.default_rng(9)
    keys, vals = draw(rng, case, 700)
    keys[rng.permutation(700)[:300]] = case["first"] + 77
    (s, o), (t, _), co = pair(case, oracle), pair(case, oracle), Coalescer(0)
    try:
        co.set_long_min(4)
        push(s, co, keys, vals, 12)
        assert co.route()[0] > 1
        co.set_long_min(0)  # the default 512: no segment is that long
        push(t, co, keys, vals, 12)
        assert host_push(o, case, keys, vals) == 0
        assert state(s, case) == state(t, case) == ostate(o, case)
    finally:
        co.close(), s.close(), t.close()


@pytest.mark.parametrize("span", [ROWS, 40], ids=["range-holds", "range-violated"])
def test_declared_range(span, oracle):
    """The coalescer's own order stage, and its fallback when a key lies outside the declared range."""
    from distml_amd import Coalescer
    case, rng = F32(50), np.random.default_rng(3)
    (s, o), co = pair(case, oracle), Coalescer(0)
    try:
        co.set_key_range(case["first"], case["first"] + span)
        keys, vals = draw(rng, case, 900)
        push(s, co, keys, vals)
        assert co.order_route()[0] == (span == ROWS)
        assert host_push(o, case, keys, vals) == 0 and state(s, case) == ostate(o, case)
    finally:
        co.close(), s.close()


def test_adagrad_values(oracle):
    """Deltas that cross 1.0, a NaN and an Inf gradient, and two elements tying for maxDelta in
    different rows (the higher row first in the list); two calls, so the running record is met."""
    from distml_amd import Coalescer
    case, rng = ADA(5), np.random.default_rng(21)
    (s, o), co = pair(case, oracle), Coalescer(0)
    try:
        keys, vals = draw(rng, case, 63)
        vals *= 1.5
        keys[np.isin(keys, case["first"] + np.array([100, 200]))] = case["first"] + 5
        keys[:2] = case["first"] + 200, case["first"] + 100
        vals[:2, 3] = 30.0  # 900.0 twice, nothing else as large: row 100 wins
        push(s, co, keys, vals)
        assert host_push(o, case, keys, vals) == 0 and state(s, case) == ostate(o, case)
        assert o.max_delta() == (900.0, int(np.int64(case["first"] + 100).astype(np.int32)), 3)
        keys, vals = draw(rng, case, 65)
        vals[5, 1], vals[9, 2] = np.nan, np.inf
        push(s, co, keys, vals, 12)
        assert host_push(o, case, keys, vals) == 0 and state(s, case) == ostate(o, case)
        assert np.isinf(o.max_delta()[0]) and (o.delta > 1.0).any() and (o.delta < 1.0).any()
    finally:
        co.close(), s.close()


@pytest.mark.parametrize("case", [F32(50), ADA(200)], ids=lambda c: c["id"])
def test_ordering_without_flush(case, oracle):
    """pushDevice(records), a plane push, a plane fetch and a second plane push on a side stream, no
    flush: the fetch sees the first two and not the last."""
    from distml_amd import Coalescer, DeviceKeys
    rng = np.random.default_rng(14)
    (s, o), co, st = pair(case, oracle), Coalescer(0), torch.cuda.Stream()
    try:
        asc = case["first"] + np.arange(ROWS, dtype=np.int64)
        rec = cc.pack_expected(case, asc, (rng.standard_normal((ROWS, case["cols"])) * 0.6).astype(np.float32))
        (k1, v1), (k2, v2), fk = draw(rng, case, 900), draw(rng, case, 900), rng.integers(0, ROWS, size=500)
        dfk = torch.from_numpy(case["first"] + fk.astype(np.int64)).cuda()
        got = torch.empty((500, case["cols"]), dtype=torch.float32, device="cuda")
        pa = geom.pack([rec], 4)
        s.pushDevice(pa.ptrs, pa.lens)
        keep = [push(s, co, k1, v1, stream=st.cuda_stream)]
        s.handleFetchPlanesDevice(s.format, DeviceKeys(dfk.data_ptr(), 500), got.data_ptr(), None, stream=st.cuda_stream)
        keep.append(push(s, co, k2, v2, stream=st.cuda_stream))
        assert o.push(rec) == 0 and host_push(o, case, k1, v1) == 0
        want = o.data[fk].tobytes()
        assert host_push(o, case, k2, v2) == 0
        s.flush()
        st.synchronize()
        assert got.cpu().numpy().tobytes() == want and state(s, case) == ostate(o, case)
    finally:
        co.close(), s.close()


@pytest.mark.parametrize("case", [F32(50), ADA(3)], ids=lambda c: c["id"])
@pytest.mark.parametrize("low", [True, False], ids=["below-first", "above-last"])
def test_keys_outside_the_shard(case, low, oracle):
    """first - 1 in the list: nothing is applied. last + 1 and last + 5: every other key is applied.
    The lowest bad key is reported (synchronous: by the call; stream: by the flush) and later pushes are
    refused until clear_error; the oracle holds the same error and the same bytes after the record push."""
    from distml_amd import ArrayIndexOutOfBoundsException, Coalescer
    rng = np.random.default_rng(33)
    (s, o), co, st = pair(case, oracle), Coalescer(0), torch.cuda.Stream()
    try:
        keys, vals, keep = *draw(rng, case, 65), None
        keys[[40, 7]] = case["first"] + ROWS + 4, case["first"] + ROWS
        if low:
            keys[11] = case["first"] - 1
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            keep = push(s, co, keys, vals, stream=None if low else st.cuda_stream)
            s.flush()
        assert host_push(o, case, keys, vals) != 0
        assert (e.value.code, e.value.key, e.value.col) == o.error() == s.error_state()
        good = draw(rng, case, 63)
        with pytest.raises(ArrayIndexOutOfBoundsException):
            push(s, co, *good)
        s.clear_error(), o.clear_error()
        assert state(s, case) == ostate(o, case)
        push(s, co, *good)
        assert host_push(o, case, *good) == 0 and state(s, case) == ostate(o, case)
    finally:
        co.close(), s.close()


def test_refusals(oracle):
    """Every refusal of the header, each with nothing launched and the shard as it was; n == 0 is DML_OK."""
    from distml_amd import Coalescer, _lib
    L, vp = _lib.load(), lambda x: C.c_void_p(x or None)  # noqa: E731
    case = F32(5)
    (s, o), co = pair(case, oracle), Coalescer(0)
    ints = [make_store(c, fc.build_init(c)) for c in (fc._case("i32", 1, 0, 0, 5, ROWS, 1000), fc._case("ai32", 0, 0, 0, 1, ROWS, 1000))]
    try:
        keys, vals = draw(np.random.default_rng(1), case, 9)
        dk, a = torch.from_numpy(keys).cuda(), geom.pack([vals.tobytes()], 4)
        k, v, c, h = dk.data_ptr(), a.ptrs[0], co._h, s._h
        before = [x.values().tobytes() for x in [s] + ints]
        bad = [("null store", (None, c, k, 9, v)), ("null coalescer", (h, None, k, 9, v)), ("n < 0", (h, c, k, -1, v)),
               ("n = 2^31", (h, c, k, 1 << 31, v)), ("null keys", (h, c, 0, 9, v)), ("null values", (h, c, k, 9, 0)),
               ("keys + 4", (h, c, k + 4, 8, v)), ("values + 2", (h, c, k, 9, v + 2))]
        other = Coalescer(1) if torch.cuda.device_count() > 1 else None
        if other:
            bad.append(("coalescer of another device", (h, other._h, k, 9, v)))
        for what, (hh, cc_, kk, n, vv) in bad:
            assert L.dml_store_push_planes_device(hh, cc_, vp(kk), n, vp(vv), None) == _lib.DML_E_INVALID_ARG, what
        for x in ints:
            assert L.dml_store_push_planes_device(x._h, c, vp(k), 9, vp(v), None) == _lib.DML_E_UNSUPPORTED
        assert L.dml_store_push_planes_device(h, c, None, 0, None, None) == 0
        assert [x.values().tobytes() for x in [s] + ints] == before and all(x.error_state()[0] == 0 for x in [s] + ints)
        push(s, co, keys, vals)
        assert host_push(o, case, keys, vals) == 0 and state(s, case) == ostate(o, case)
        other and other.close()
    finally:
        co.close(), s.close(), [x.close() for x in ints]

"""Device-resident handleFetch (dml_store_fetch_device / _fetch_range_device,
DataStore.handleFetchDevice) against the CPU oracle's fetch, byte for byte.

Every fetch writes into a geom.OutArena: the output sits at base + GUARD + lead inside a
poison word, at all four leads (0, 4, 8, 12 mod 16), the arena is read back, the output
region is compared with oracle.fetch(keys), and every byte outside it must still be poison.
The cases are tests/fetch_cases.py (pinned on the CPU by test_fetch_device_cases.py).

Every case runs with DML_KNOB_FETCH_KERNEL = 2, which proves k_fetch_vec ran (the call
would return DML_E_UNSUPPORTED for a shape that kernel did not take). The default dispatch
(0) picks k_fetch_vec for every shape too, so it differs nowhere; test_layouts runs it
once per case at one lead all the same, and test_both_kernels_agree compares with k_fetch
(knob 1).
"""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KNOB = 3      # DML_KNOB_FETCH_KERNEL
K_FETCH, K_VEC = 1, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def make_store(case, init=None, knob=K_VEC, first_push=True):
    """The GPU store of a case, set up as fc.make_oracle sets up the oracle."""
    from distml_amd import DataDesc, DataStore, KeyRange
    fmt = DataDesc(case["dt"], case["kt"], case["vt"], False, True, case["ada"])
    s = DataStore(fmt, KeyRange(case["first"], case["first"] + case["rows"] - 1), case["cols"],
                  float_array_ref_stride=case["ref_stride"])
    s.set_knob(KNOB, knob)
    if case["ada"]:
        s.setAlpha(*fc.ADA)
    s.load_values(fc.build_init(case) if init is None else init)
    if case["ada"] and first_push:
        s.handlePush(fmt, fc.ada_push(case))
    return s


def dev_keys(keys):
    from distml_amd import DeviceKeys
    t = torch.from_numpy(np.ascontiguousarray(keys, np.int64).copy()).cuda() if len(keys) else \
        torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return t, DeviceKeys(t.data_ptr(), len(keys))


def zero_push(case):
    from distml_amd.store import encode_array_push, encode_matrix_push
    if case["dt"] == 1:
        return encode_matrix_push([case["first"]], np.zeros((1, case["cols"]), fc.VDT[case["vt"]]), case["kt"], case["vt"])
    return encode_array_push([case["first"]], np.zeros(1, fc.VDT[case["vt"]]), case["kt"], case["vt"],
                             8 if case["ref_stride"] else None)


def raw_fetch(s, keys_ptr, n, out_ptr, cap, stream=None):
    """The C call itself: (status, out_len)."""
    from distml_amd import _lib
    ln = C.c_int64(-7)
    rc = _lib.load().dml_store_fetch_device(s._h, C.c_void_p(keys_ptr or None), n, C.c_void_p(out_ptr or None), cap,
                                            C.byref(ln), C.c_void_p(stream or None))
    return rc, ln.value


def fetch_check(s, rows, want, lead, what):
    """One synchronous fetch into a fresh arena: bytes equal `want`, nothing else written."""
    a = geom.OutArena(len(want), lead).upload()
    n = s.handleFetchDevice(s.format, rows, a.ptr, len(want))
    assert n == len(want), (what, n, len(want))
    got = a.read()
    if got.tobytes() != want:
        bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
        raise AssertionError((what, "first differing byte", int(bad[0]), "of", len(want), "count", int(bad.size)))
    a.untouched([(0, n)])


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c["id"])
def test_layouts(oracle, case):
    """Test 1. The four matrix stores (AdaGrad after setAlpha and one push) at 1, 3, 4, 5, 17,
    50, 200, 256, 1000, 1023 and 1025 columns, the three array stores and FloatArrayStore with
    DML_FLAG_FLOAT_ARRAY_REF_STRIDE, int32 and int64 keys, first keys 1000 / BIG33 / STRADDLE /
    NEG32, initial values with -0.0, denormals, +-Inf and NaN payloads. Lists: all rows
    ascending, a shuffled subset with repeats, one key, no key. Ranges: whole, sticking out on
    both sides, inner, clipped on one side, one row, disjoint. Each at the four leads."""
    from distml_amd import KeyRange
    recs = {fc.record_bytes(c) % 16 for c in fc.CASES if c["store"] == case["store"] and c["dt"] == 1}
    assert case["dt"] == 0 or recs == {0, 4, 8, 12}
    _, o = fc.make_oracle(case, oracle)
    s = make_store(case)
    try:
        lists = {k: (v, o.fetch(v)) for k, v in fc.key_lists(case).items()}
        rngs = {k: (a, b, o.fetch(keys)) for k, (a, b, keys) in fc.ranges(case).items()}
        for lead in geom.LEADS:
            for name, (keys, want) in lists.items():
                t, dk = dev_keys(keys)
                fetch_check(s, dk, want, lead, (case["id"], "list", name, lead))
            for name, (a, b, want) in rngs.items():
                fetch_check(s, KeyRange(a, b), want, lead, (case["id"], "range", name, lead))
        s.set_knob(KNOB, 0)  # the default dispatch
        t, dk = dev_keys(lists["shuffled"][0])
        fetch_check(s, dk, lists["shuffled"][1], 4, (case["id"], "dispatch list"))
        fetch_check(s, KeyRange(*rngs["inner"][:2]), rngs["inner"][2], 12, (case["id"], "dispatch range"))
        assert s.error_state()[0] == 0
    finally:
        s.close()


def test_tiling_edges(oracle):
    """Test 2. k_fetch_vec's tiles: DML_FETCH_WAVE_BYTES = 1 024 (one wave instruction's 64
    16-byte vectors) and DML_FETCH_BLOCK_BYTES = 4 096 (a block's 256 vectors). With 24-byte
    records (5 f32 columns, int32 keys) the stream ends one record before, exactly at and one
    record past three whole wave runs (383, 384, 385 keys) and three whole blocks (511, 512,
    513 keys); list and range form, four leads (a lead moves every vector boundary by 4, 8
    or 12 bytes against the records). The four-vectors-per-thread shape (16-KiB blocks, knob
    bit 4096) runs the same counts plus its own block edge (2 047, 2 048, 2 049 keys)."""
    from distml_amd import KeyRange, _lib
    case = fc.EDGE_CASE
    ns = fc.edge_counts(_lib.DML_FETCH_WAVE_BYTES, _lib.DML_FETCH_BLOCK_BYTES)
    assert ns == [383, 384, 385, 511, 512, 513]
    _, o = fc.make_oracle(case, oracle)
    s = make_store(case)
    try:
        rng = np.random.default_rng(5)
        for n in ns + [-2047, -2048, -2049]:
            s.set_knob(KNOB, K_VEC | (16 << 8 if n < 0 else 0))
            n = abs(n)
            asc = case["first"] + np.arange(n, dtype=np.int64)
            perm = case["first"] + rng.permutation(case["rows"])[:n].astype(np.int64)
            want_asc, want_perm = o.fetch(asc), o.fetch(perm)
            t, dk = dev_keys(perm)
            for lead in geom.LEADS:
                fetch_check(s, KeyRange(int(asc[0]), int(asc[-1])), want_asc, lead, ("edge range", n, lead))
                fetch_check(s, dk, want_perm, lead, ("edge list", n, lead))
    finally:
        s.close()


class _Raw:
    """A device allocation as torch sees foreign memory."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr=typestr, data=(ptr, False), version=2)


def test_output_past_4_gib():
    """Test 3. One f32 range fetch of 5.4 M x 200 (4.34 GB of output: byte offsets pass 2^32),
    compared on the device: column 0 of the int32 view is first + arange, the rest is the
    shard's bits. No host copy of the output."""
    from distml_amd import DataDesc, DataStore, KeyRange
    rows, cols, first = 5_400_000, 200, 1000
    assert rows * (4 + 4 * cols) > 1 << 32
    s = DataStore(DataDesc(1, 0, 1), KeyRange(first, first + rows - 1), cols)
    try:
        s.set_knob(KNOB, K_VEC)
        s.rand(3)
        out = torch.full((rows * (1 + cols) + 2,), geom.poison_i32(), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the fetch on the store's
        n = s.handleFetchDevice(s.format, KeyRange(first, first + rows - 1), out.data_ptr() + 4, 4 * (out.numel() - 2))
        assert n == 4 * rows * (1 + cols)
        assert int(out[0]) == geom.poison_i32() and int(out[-1]) == geom.poison_i32()
        rec = out[1:-1].view(rows, 1 + cols)
        assert torch.equal(rec[:, 0], torch.arange(first, first + rows, dtype=torch.int32, device="cuda"))
        shard = torch.as_tensor(_Raw(s.device_ptr(), rows * cols, "<i4"), device="cuda").view(rows, cols)
        step = 600_000  # compare in slabs: the comparison's temporaries stay small
        for r0 in range(0, rows, step):
            assert torch.equal(rec[r0:r0 + step, 1:], shard[r0:r0 + step]), r0
        del shard
    finally:
        s.close()


ORDER_CASES = [fc._case("f32", 1, 0, 1, 1024, 301, 1000), fc._case("ada", 1, 0, 1, 1024, 301, 1000, True),
               fc._case("i32", 1, 0, 0, 1024, 301, 1000)]


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: c["id"])
def test_ordering_between_pushes(oracle, case):
    """Test 4. pushDevice, handleFetchDevice on a torch stream, two more pushDevice calls, with
    no synchronisation in between. 1 024 columns and ascending full-range pushes: the plain
    stores' chunks are speculative, so the push after the fetch writes the second shard
    buffer and the one after it writes back the buffer the fetch reads. The fetched bytes
    are the oracle's after the first push; after flush the store is the oracle's after all
    three."""
    from distml_amd import KeyRange
    from distml_amd.store import encode_matrix_push
    rng = np.random.default_rng(77)
    rows, cols, first = case["rows"], case["cols"], case["first"]
    init = rng.integers(100, 200, size=(rows, cols)).astype(np.int32) if case["vt"] == 0 else \
        rng.standard_normal((rows, cols)).astype(np.float32)
    pushes = []
    for b in range(3):
        v = rng.integers(-2, 3, size=(rows, cols)).astype(np.int32) if case["vt"] == 0 else \
            (rng.standard_normal((rows, cols)) * (0.6 if case["ada"] else 1e-3)).astype(np.float32)
        pushes.append(encode_matrix_push(first + np.arange(rows, dtype=np.int64), v, case["kt"], case["vt"]))
    o = oracle.OracleStore(1, case["kt"], case["vt"], first, first + rows - 1, cols, 1, int(case["ada"]), 0)
    if case["ada"]:
        o.set_alpha(*fc.ADA)
    o.data[:] = init
    assert o.push(pushes[0]) == 0
    want = o.fetch(first + np.arange(rows, dtype=np.int64))
    assert o.push(pushes[1]) == 0 and o.push(pushes[2]) == 0
    s = make_store(case, init, first_push=False)
    try:
        arenas = [geom.pack([p], 4) for p in pushes]
        out = geom.OutArena(len(want), 8).upload()
        st = torch.cuda.Stream()
        s.stats(reset=True)
        s.pushDevice(arenas[0].ptrs, arenas[0].lens)
        n = s.handleFetchDevice(s.format, KeyRange(first, first + rows - 1), out.ptr, len(want), stream=st.cuda_stream)
        s.pushDevice(arenas[1].ptrs, arenas[1].lens)
        s.pushDevice(arenas[2].ptrs, arenas[2].lens)
        st.synchronize()
        assert n == len(want)
        assert out.read().tobytes() == want
        out.untouched([(0, n)])
        s.flush()
        assert s.values().tobytes() == o.data.tobytes()
        if case["ada"]:
            al, _ = s.adagrad_state()
            assert al.tobytes() == o.alpha.tobytes()
        elif case["vt"] == 1:
            assert s.stats()["spec_chunks"] == 3  # the shape under test: both shard buffers in play
    finally:
        s.close()


def test_refusals(oracle):
    """Test 5. dev_out + 2, dev_keys + 4, a null key pointer, nkeys = -1 and cap = out_len - 4:
    each returns its code with *out_len as the header documents (nkeys x record bytes; 0 for
    nkeys < 0), the arena is wholly untouched and the store's error state stays 0. A store
    closed by a negative counter answers the device fetch as it answers dml_store_fetch."""
    from distml_amd import _lib
    case = fc._case("f32", 1, 1, 1, 5, 301, geom.BIG33)
    rec = fc.record_bytes(case)
    s = make_store(case)
    try:
        keys = case["first"] + np.arange(9, dtype=np.int64)
        t, dk = dev_keys(np.concatenate([keys, keys]))
        full = 9 * rec
        a = geom.OutArena(full, 4).upload()
        E = _lib.DML_E_INVALID_ARG
        st = torch.cuda.Stream()
        for what, args, want in (
                ("out + 2", (dk.ptr, 9, a.ptr + 2, full), (E, full)),
                ("keys + 4", (dk.ptr + 4, 9, a.ptr, full), (E, full)),
                ("null keys", (0, 9, a.ptr, full), (E, full)),
                ("nkeys -1", (dk.ptr, -1, a.ptr, full), (E, 0)),
                ("cap short", (dk.ptr, 9, a.ptr, full - 4), (_lib.DML_E_CAPACITY, full)),
                ("null out", (dk.ptr, 9, 0, full), (_lib.DML_E_CAPACITY, full))):
            for stream in (None, st.cuda_stream):
                assert raw_fetch(s, *args, stream=stream) == want, what
        assert _lib.load().dml_store_fetch_device(s._h, C.c_void_p(dk.ptr), 9, C.c_void_p(a.ptr), full, None, None) == E
        a.read()
        a.untouched([])
        assert s.error_state()[0] == 0
        assert raw_fetch(s, dk.ptr, 9, a.ptr, full) == (0, full)  # and the same arguments, in order, work
    finally:
        s.close()
    # a store closed by a negative counter
    from distml_amd.store import encode_matrix_push
    ci = fc._case("i32", 1, 0, 0, 5, 301, 1000)
    s = make_store(ci, np.ones((301, 5), np.int32))
    try:
        p = encode_matrix_push([1003], np.full((1, 5), -2, np.int32), 0, 0)
        with pytest.raises(Exception):
            s.handlePush(s.format, p)
            s.flush()
        assert s.error_state()[0] == _lib.DML_E_NEGATIVE_COUNTER
        keys = np.array([1001, 1002], np.int64)
        host = np.zeros(2 * 24, np.uint8)
        ln = C.c_int64()
        rc_host = _lib.load().dml_store_fetch(s._h, keys.ctypes.data_as(C.POINTER(C.c_int64)), 2, host.ctypes.data, 48,
                                              C.byref(ln))
        t, dk = dev_keys(keys)
        a = geom.OutArena(48, 0).upload()
        rc_dev, n = raw_fetch(s, dk.ptr, 2, a.ptr, 48)
        assert rc_dev == rc_host and n == ln.value
        if rc_host == 0:
            assert a.read().tobytes() == host.tobytes()
        assert s.error_state()[0] == _lib.DML_E_NEGATIVE_COUNTER
    finally:
        s.close()


@pytest.mark.parametrize("case", [fc._case("f32", 1, 1, 1, 50, 301, geom.STRADDLE),
                                  fc._case("ada", 1, 0, 1, 17, 301, geom.NEG32, True),
                                  fc._case("af32", 0, 1, 1, 1, 1237, geom.BIG33)], ids=lambda c: c["id"])
@pytest.mark.parametrize("knob", [K_VEC, K_FETCH])
def test_keys_outside_the_shard(oracle, case, knob):
    """Test 6. last + 1 at index 7 and first - 1 at index 3. Asynchronous form: the call
    returns DML_OK, every other record is the oracle's, the two refused records' bytes are
    still poison, and the flush (first run) or the next push (second run, issued once the
    caller's stream has passed the fetch) raises for key first - 1, col -1; the error is
    sticky, and after clear_error the store fetches correctly. Synchronous form: the call
    itself raises. An int64 alias (first + 5 + 2^32) is refused too. Both kernels."""
    from distml_amd import ArrayIndexOutOfBoundsException, _lib
    keys, bad, reported = fc.out_of_shard_plan(case)
    rec = fc.record_bytes(case)
    _, o = fc.make_oracle(case, oracle)
    good = [i for i in range(len(keys)) if i not in bad]
    want = {i: o.fetch(keys[i:i + 1]) for i in good}
    spans = [(i * rec, (i + 1) * rec) for i in good]
    s = make_store(case, knob=knob)
    st = torch.cuda.Stream()
    try:
        t, dk = dev_keys(keys)
        zero = geom.pack([zero_push(case)], 0)  # one record that adds nothing to the first row
        for run in ("flush", "push"):
            a = geom.OutArena(len(keys) * rec, 4).upload()
            rc, n = raw_fetch(s, dk.ptr, len(keys), a.ptr, len(keys) * rec, stream=st.cuda_stream)
            assert (rc, n) == (0, len(keys) * rec)
            st.synchronize()
            with pytest.raises(ArrayIndexOutOfBoundsException) as e:
                if run == "flush":
                    s.flush()
                else:
                    s.pushDevice(zero.ptrs, zero.lens)
            assert (e.value.code, e.value.key, e.value.col) == (_lib.DML_E_KEY_OUT_OF_SHARD, reported, -1)
            got = a.read()
            for i in good:
                assert got[i * rec:(i + 1) * rec].tobytes() == want[i], (run, i)
            a.untouched(spans)  # the refused records, and everything around the output: poison
            assert s.error_state() == (_lib.DML_E_KEY_OUT_OF_SHARD, reported, -1)  # sticky
            s.clear_error()
            assert s.error_state()[0] == 0
            gk = keys[good]
            t2, dk2 = dev_keys(gk)
            fetch_check(s, dk2, o.fetch(gk), 8, ("after clear_error", run))
        # synchronous: the call itself
        a = geom.OutArena(len(keys) * rec, 12).upload()
        rc, n = raw_fetch(s, dk.ptr, len(keys), a.ptr, len(keys) * rec)
        assert (rc, n) == (_lib.DML_E_KEY_OUT_OF_SHARD, len(keys) * rec)
        assert s.error_state() == (_lib.DML_E_KEY_OUT_OF_SHARD, reported, -1)
        a.read()
        a.untouched(spans)
        s.clear_error()
        if case["kt"] == 1:
            alias = np.array([case["first"] + 1, case["first"] + 5 + geom.ALIAS, case["first"] + 2], np.int64)
            t3, dk3 = dev_keys(alias)
            a = geom.OutArena(3 * rec, 0).upload()
            rc, n = raw_fetch(s, dk3.ptr, 3, a.ptr, 3 * rec)
            assert rc == _lib.DML_E_KEY_OUT_OF_SHARD and s.error_state()[1] == int(alias[1])
            got = a.read()
            assert got[:rec].tobytes() == o.fetch(alias[:1]) and got[2 * rec:].tobytes() == o.fetch(alias[2:])
            a.untouched([(0, rec), (2 * rec, 3 * rec)])
            s.clear_error()
    finally:
        s.close()


ROUND_TRIP = [fc._case("f32", 1, 0, 1, 200, 1237, geom.NEG32), fc._case("i32", 1, 1, 0, 17, 1237, geom.BIG33),
              fc._case("f64", 1, 1, 3, 50, 1237, geom.STRADDLE), fc._case("ai32", 0, 0, 0, 1, 1237, 1000),
              fc._case("af64", 0, 1, 3, 1, 1237, geom.BIG33),
              fc._case("af32ref", 0, 0, 1, 1, 1237, 1000, False, True)]


@pytest.mark.parametrize("case", ROUND_TRIP, ids=lambda c: c["id"])
def test_round_trip_into_push_device(case):
    """Test 7. The whole range of store A fetched on the device and handed to pushDevice of a
    zeroed store B of the same shape: B's bytes equal A's. Plain f32 / i32 / f64 matrices and
    the int and double arrays, whose fetched record is byte for byte a push record. The
    float array only with DML_FLAG_FLOAT_ARRAY_REF_STRIDE: FloatArrayStore fetches 8-byte
    value slots, and only with that flag does its push read records of that stride (without
    it a push record is [key][4-byte value], and a fetch is not one). Values without -0.0
    and NaN: B adds them to zero."""
    from distml_amd import KeyRange
    init = fc.build_init(case, plain=True)
    if case["vt"] == 0:
        init = np.abs(init // 2)  # int32 counters stay non-negative (IntMatrixStore's check)
    a = make_store(case, init)
    b = make_store(case, np.zeros_like(init))
    try:
        n = fc.record_bytes(case) * case["rows"]
        buf = geom.OutArena(n, 12).upload()
        st = torch.cuda.Stream()
        whole = KeyRange(case["first"], case["first"] + case["rows"] - 1)
        assert a.handleFetchDevice(a.format, whole, buf.ptr, n, stream=st.cuda_stream) == n
        st.synchronize()  # B's apply stream is not the caller's: the caller orders the two
        b.pushDevice([buf.ptr], [n])
        b.flush()
        assert b.values().tobytes() == a.values().tobytes() == init.tobytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("case", [fc._case("f32", 1, 0, 1, 200, 1237, 1000),
                                  fc._case("ada", 1, 1, 1, 48, 1237, geom.BIG33, True),
                                  fc._case("af64", 0, 1, 3, 1, 1237, geom.STRADDLE)], ids=lambda c: c["id"])
def test_both_kernels_agree(oracle, case):
    """Test 8. DML_KNOB_FETCH_KERNEL 1 (k_fetch) and 2 (k_fetch_vec, and its other launch
    shapes: bits 8-12) write the same bytes: 200 columns f32, AdaGrad 48 columns, the f64 array."""
    from distml_amd import KeyRange
    _, o = fc.make_oracle(case, oracle)
    s = make_store(case)
    try:
        keys = fc.key_lists(case)["shuffled"]
        want_l = o.fetch(keys)
        a0, b0, rk = fc.ranges(case)["inner"]
        want_r = o.fetch(rk)
        t, dk = dev_keys(keys)
        for knob in (K_FETCH, K_VEC, *(K_VEC | v << 8 for v in (1, 2, 4, 8, 16, 5, 14, 22))):
            s.set_knob(KNOB, knob)
            fetch_check(s, dk, want_l, 4, ("agree list", knob))
            fetch_check(s, KeyRange(a0, b0), want_r, 8, ("agree range", knob))
        from distml_amd.store import NativeError
        with pytest.raises(NativeError):
            s.set_knob(KNOB, 3)
        with pytest.raises(NativeError):
            s.set_knob(KNOB, K_VEC | 24 << 8)
    finally:
        s.close()

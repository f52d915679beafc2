"""dml_store_fetch_planes_device: row j of the planes is the shard row of key j, byte for byte, against
numpy on what the store itself reports (values()[keys - first], adagrad_state()'s alpha). Planes sit in
geom.OutArena poison at 4 (values) and 12 (alpha) mod 16; every byte outside them must still be poison."""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom
from test_gpu_worker_iteration import _gpu, make_store  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 301
# rows of 12 B (the narrow kernel's last), 16 B, 20 and 200 B (ragged), 1 KiB and 1 KiB + 4; f64: 8 B, 16 B, 1 KiB + 8
F32_COLS, F64_COLS = (1, 3, 4, 5, 50, 256, 257), (1, 2, 129)
CASES = ([fc._case("f32", 1, 0, 1, c, ROWS, geom.NEG32) for c in F32_COLS] +
         [fc._case("ada", 1, 1, 1, c, ROWS, geom.BIG33, True) for c in F32_COLS] +
         [fc._case("f64", 1, 1, 3, c, ROWS, geom.STRADDLE) for c in F64_COLS] +
         [fc._case("i32", 1, 0, 0, 1000, ROWS, 1000), fc._case("ai32", 0, 0, 0, 1, ROWS, geom.NEG32),
          fc._case("af32", 0, 1, 1, 1, ROWS, geom.BIG33), fc._case("af64", 0, 1, 3, 1, ROWS, geom.STRADDLE)])


def store_of(case):
    s = make_store(case, fc.build_init(case))
    case["ada"] and s.handlePush(s.format, fc.ada_push(case))  # alpha and values vary by row
    return s


def call(s, keys_ptr, n, values_ptr, alpha_ptr=0, stream=None):
    from distml_amd import _lib
    vp = lambda x: C.c_void_p(x or None)  # noqa: E731
    return _lib.load().dml_store_fetch_planes_device(s._h, vp(keys_ptr), n, vp(values_ptr), vp(alpha_ptr), vp(stream))


def reference(s, case, keys):
    idx = keys - case["first"]
    planes = [np.asarray(s.values()).reshape(ROWS, -1)[idx]]
    return planes + [s.adagrad_state()[0][idx]] if case["ada"] else planes


def fetch_and_check(s, keys, want, good=None, stream=None, before=None, after=None):
    """One fetch (`before` and `after` run around it): rows `good` (default: all) equal `want`, nothing else is written."""
    n = len(keys)
    good = np.arange(n) if good is None else np.asarray(good)
    arenas = [geom.OutArena(n * w[0].nbytes, lead).upload() for w, lead in zip(want, (4, 12))]
    dk = torch.from_numpy(np.ascontiguousarray(keys, np.int64).copy()).cuda()
    torch.cuda.synchronize()
    before and before()
    rc = call(s, dk.data_ptr(), n, *(a.ptr for a in arenas), stream=stream)
    after and after()
    for a, w in zip(arenas, want):
        row = w[0].nbytes
        assert a.read().reshape(n, row)[good].tobytes() == w.tobytes(), n
        a.untouched([(int(i) * row, int(i + 1) * row) for i in good])
    return rc


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_bytes(case):
    """All seven store kinds; n = 1, 63, 65 and 900 drawn from the shard's 301 rows, in arbitrary
    order; n = 900 also at every depth of DML_KNOB_FETCH_PLANES (knob 4)."""
    rng = np.random.default_rng(len(case["id"]) + case["cols"])
    s = store_of(case)
    try:
        for n, depth in ((1, 0), (63, 0), (65, 0), (900, 0), (900, 1), (900, 2), (900, 4)):
            keys = case["first"] + rng.integers(0, ROWS, size=n).astype(np.int64)
            keys[0], keys[-1] = case["first"], case["first"] + ROWS - 1
            s.set_knob(4, depth)
            assert fetch_and_check(s, keys, reference(s, case, keys)) == 0 and s.error_state()[0] == 0
    finally:
        s.close()


@pytest.mark.parametrize("case", [fc._case("ada", 1, 1, 1, 50, ROWS, geom.BIG33, True),
                                  fc._case("ada", 1, 0, 1, 3, ROWS, geom.NEG32, True)], ids=lambda c: c["id"])
def test_refused_keys(case):
    """last + 1 at index 7 and first - 1 at index 3: both rows keep their poison in both planes,
    every other row is right; the synchronous call returns DML_E_KEY_OUT_OF_SHARD and the state
    names first - 1; the stream form reports at flush; clear_error lets the next call through."""
    from distml_amd import ArrayIndexOutOfBoundsException, _lib
    keys, bad, reported = fc.out_of_shard_plan(case)
    good = [i for i in range(len(keys)) if i not in bad]
    E = (_lib.DML_E_KEY_OUT_OF_SHARD, reported, -1)
    s, st = store_of(case), torch.cuda.Stream()
    try:
        want = reference(s, case, keys[good])
        assert fetch_and_check(s, keys, want, good) == E[0] and s.error_state() == E
        s.clear_error()
        assert fetch_and_check(s, keys, want, good, stream=st.cuda_stream) == 0
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            s.flush()
        assert (e.value.code, e.value.key, e.value.col) == E and s.error_state() == E
        s.clear_error()
        assert fetch_and_check(s, keys[good], want) == 0 and s.error_state()[0] == 0
    finally:
        s.close()


@pytest.mark.parametrize("case", [fc._case("f32", 1, 0, 1, 1024, ROWS, 1000),
                                  fc._case("ada", 1, 0, 1, 200, ROWS, 1000, True)], ids=lambda c: c["id"])
def test_ordering_between_pushes(case):
    """pushDevice A, fetch planes on a torch stream, pushDevice B, no flush: the planes hold the
    state after A (a twin store given A alone) and before B."""
    from distml_amd.store import encode_matrix_push
    rng = np.random.default_rng(78)
    first, cols, asc = case["first"], case["cols"], case["first"] + np.arange(ROWS, dtype=np.int64)
    init = rng.standard_normal((ROWS, cols)).astype(np.float32)
    A, B = (encode_matrix_push(asc, (rng.standard_normal((ROWS, cols)) * 0.6).astype(np.float32), 0, 1) for _ in "AB")
    s, twin, st = make_store(case, init), make_store(case, init), torch.cuda.Stream()
    try:
        twin.handlePush(twin.format, A)
        keys = first + rng.integers(0, ROWS, size=900).astype(np.int64)
        pa, pb = geom.pack([A], 4), geom.pack([B], 4)
        assert fetch_and_check(s, keys, reference(twin, case, keys), stream=st.cuda_stream,
                               before=lambda: s.pushDevice(pa.ptrs, pa.lens),
                               after=lambda: s.pushDevice(pb.ptrs, pb.lens)) == 0
        s.flush()
        twin.handlePush(twin.format, B)
        assert s.values().tobytes() == twin.values().tobytes()
    finally:
        s.close()
        twin.close()


def test_arguments():
    """Each refusal: DML_E_INVALID_ARG, nothing written, store state unchanged; n == 0 is DML_OK; the next fetch is exact."""
    from distml_amd import _lib
    case, ada = fc._case("f32", 1, 0, 1, 5, ROWS, 1000), fc._case("ada", 1, 0, 1, 5, ROWS, 1000, True)
    s, sa = store_of(case), store_of(ada)
    try:
        keys = case["first"] + np.arange(9, dtype=np.int64)
        dk = torch.from_numpy(keys).cuda()
        k, a, b = dk.data_ptr(), geom.OutArena(9 * 20, 4).upload(), geom.OutArena(9 * 20, 12).upload()
        for what, st, args in (("n < 0", s, (k, -1, a.ptr)), ("null keys", s, (0, 9, a.ptr)), ("null values", s, (k, 9, 0)),
                               ("keys + 4", s, (k + 4, 8, a.ptr)), ("values + 2", s, (k, 9, a.ptr + 2)),
                               ("alpha + 2", sa, (k, 9, a.ptr, b.ptr + 2)), ("alpha, not AdaGrad", s, (k, 9, a.ptr, b.ptr)),
                               ("values on keys", s, (k, 9, k + 8)), ("alpha on keys", sa, (k, 9, a.ptr, k + 64)),
                               ("planes overlap", sa, (k, 9, a.ptr, a.ptr + 9 * 20 - 4))):
            assert call(st, *args) == _lib.DML_E_INVALID_ARG, what
        assert call(s, k, 0, a.ptr) == 0
        for x in (a, b):
            x.read()
            x.untouched([])
        assert dk.cpu().numpy().tobytes() == keys.tobytes() and s.error_state()[0] == sa.error_state()[0] == 0
        for st, c in ((s, case), (sa, ada)):
            assert fetch_and_check(st, keys, reference(st, c, keys)) == 0
    finally:
        s.close()
        sa.close()

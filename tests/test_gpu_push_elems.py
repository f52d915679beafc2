"""dml_store_push_elems_device (DataStore.handlePushElemsDevice): element updates straight into the int32
stores. Every comparison is byte equality of the store (values and error state) with the CPU oracle fed
the host worker's push: np.add.at mod 2^32 per distinct key, keys sorted, encode_matrix_push (arrays:
encode_array_push). Inputs sit in geom.Arena poison at 4 or 12 mod 16 and must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom
from test_gpu_coalesce_elems import NEVER, SLICE, _gpu, co, expect, moves  # noqa: F401  (_gpu: the GPU gate)
from test_gpu_worker_iteration import make_store

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from distml_amd import DeviceKeys, DistMLException, _lib, encode_array_push, encode_matrix_push  # noqa: E402

ROWS, FIRST, INT_MAX = 320, {0: geom.NEG32, 1: geom.BIG33}, 2 ** 31 - 1
MAT = lambda kt, cols, rows=ROWS: fc._case("i32", 1, kt, 0, cols, rows, FIRST[kt])  # noqa: E731
ARR = lambda kt: fc._case("ai32", 0, kt, 0, 1, ROWS, FIRST[kt])  # noqa: E731


def pair(case, oracle, init):
    o = oracle.OracleStore(case["dt"], case["kt"], 0, case["first"], case["first"] + case["rows"] - 1, case["cols"], 1, 0, 0)
    o.data[:] = init
    return make_store(case, init), o


def state(s):
    e = s.error_state()
    return s.values().tobytes(), e if e[0] else (0, 0, -1)


def ostate(o):
    e = o.error()
    return o.data.tobytes(), e if e[0] else (0, 0, -1)


def push(s, co, keys, c, v, lead=4, stream=None):
    """One element push; returns the arenas, which must stay alive until the apply stream has passed it."""
    ar = [geom.pack([keys.tobytes()], lead & 8), c is not None and geom.pack([c.tobytes()], lead), geom.pack([v.tobytes()], 16 - lead)]
    s.handlePushElemsDevice(s.format, co, DeviceKeys(ar[0].ptrs[0], len(keys)), ar[1] and ar[1].ptrs[0], ar[2].ptrs[0],
                            v.shape[1], stream=stream)
    return [a for a in ar if a]


def host_push(case, keys, c, v):
    """The host worker's push of the same moves."""
    if case["dt"]:
        return expect(keys, c, v, case["cols"], case["kt"], True)[2]
    uk, inv = np.unique(keys, return_inverse=True)
    tot = np.zeros(len(uk), np.int64)
    np.add.at(tot, inv, v.astype(np.int64).sum(axis=1))
    return encode_array_push(uk, (tot & 0xFFFFFFFF).astype(np.uint32).view(np.int32), case["kt"], 0)


def shard_moves(case, n, per, seed):
    """moves() with its keys mapped one to one onto shuffled shard rows and its deltas scaled to 2^18, so
    that counters drawn in [2^29, 2^30) stay positive over a test's calls (the oracle's rc asserts it)."""
    keys, c, v = moves(n, case["cols"], per, seed)
    uk, inv = np.unique(keys, return_inverse=True)
    rows = np.random.default_rng(seed).permutation(ROWS)[:len(uk)]
    return case["first"] + rows[inv].astype(np.int64), c, v >> 12


@pytest.mark.parametrize("kt", [0, 1], ids=["k4", "k8"])
@pytest.mark.parametrize("per", [1, 2, 16])
@pytest.mark.parametrize("cols", [1, 3, 250, 1000, SLICE, SLICE + 1, 2 * SLICE + 3])
def test_parity(co, oracle, cols, per, kt):
    """n = 1, 63, 64, 65 and 3 000 on one store. Per n: the call on the short route, a record push, a
    plane fetch and the same call on the long route (long_min 2), on a side stream with no flush."""
    case, rng, st = MAT(kt, cols), np.random.default_rng(cols + per), torch.cuda.Stream()
    s, o = pair(case, oracle, rng.integers(2 ** 29, 2 ** 30, size=(ROWS, cols)).astype(np.int32))
    try:
        for i, n in enumerate([1, 63, 64, 65, 3000]):
            keys, c, v = shard_moves(case, n, per, seed=cols + per + i)
            host, longs = host_push(case, keys, c, v), expect(keys, c, v, cols, kt, True)[3]
            fk = rng.integers(0, ROWS, size=50)
            rec = encode_matrix_push(case["first"] + np.arange(ROWS), rng.integers(0, 9, size=(ROWS, cols)).astype(np.int32), kt, 0)
            dfk, pa = torch.from_numpy(case["first"] + fk.astype(np.int64)).cuda(), geom.pack([rec], 4)
            got = torch.empty((50, cols), dtype=torch.int32, device="cuda")
            co.set_long_min(NEVER)
            keep = push(s, co, keys, c, v, (4, 12)[i % 2], st.cuda_stream)
            assert co.route() == (0, 0), n
            s.pushDevice(pa.ptrs, pa.lens)
            s.handleFetchPlanesDevice(s.format, DeviceKeys(dfk.data_ptr(), 50), got.data_ptr(), None, stream=st.cuda_stream)
            co.set_long_min(2)
            keep += push(s, co, keys, c, v, (12, 4)[i % 2], st.cuda_stream)
            assert co.route() == longs, n
            assert o.push(host) == 0 and o.push(rec) == 0
            want = o.data[fk].tobytes()
            assert o.push(host) == 0
            s.flush()
            st.synchronize()
            assert got.cpu().numpy().tobytes() == want and state(s) == ostate(o), n
            [a.check() for a in keep]
    finally:
        co.set_long_min(0)
        s.close()


W = SLICE + 8  # two slices per row
# (id, long_min, counters preset as (row, col, value), occurrences (row, col, delta) in list order); every
# other counter starts at 5. Rows are shard rows; row 40 is last + 1 and row -1 is first - 1.
VERDICTS = [
    ("col0-of-lowest-key", NEVER, [], [(7, 0, -9), (3, 5, 1), (3, 0, -6), (7, 2, 1), (9, 1, 1)]),
    ("slice-edge-lower-wins", NEVER, [], [(4, SLICE, -6), (4, SLICE - 1, -6), (4, W - 1, 1), (4, 0, 1)]),
    ("lower-key-later-in-list", NEVER, [], [(9, 1, -6), (12, 3, 1), (2, 8, -6), (2, 9, 1)]),
    ("fails-long-later-short", 3, [], [(2, 7, -2)] * 4 + [(1, 0, 1), (5, 3, 1), (6, SLICE + 2, 1)]),
    ("fails-short-later-long", 3, [], [(2, 7, -6)] + [(6, SLICE + 2, 1)] * 4 + [(1, 1, 1)] * 3),
    ("int-max-plus-one", NEVER, [(3, 4, INT_MAX)], [(3, 4, 1), (3, 5, 1), (8, 0, 1)]),
    ("zero-update-over-negative", NEVER, [(6, 9, -3)], [(6, -1, 4), (8, 1, 1), (5, 0, 1)]),
    ("dip-ends-nonnegative", NEVER, [], [(3, 0, -9), (3, 0, 9), (3, 1, -5)]),
    ("key-below-first", NEVER, [], [(5, 1, 1), (-1, 0, 1), (6, 2, 1)]),
    ("key-above-last", NEVER, [], [(41, 1, 1), (5, 1, 1), (40, 0, 1), (39, W - 1, 1)]),
    ("key-above-last-and-negative", 2, [], [(40, 0, 1), (5, 1, -6), (39, 2, 1), (39, 2, 1)]),
]


@pytest.mark.parametrize("name,lmin,preset,occ", VERDICTS, ids=[v[0] for v in VERDICTS])
def test_verdicts(co, oracle, name, lmin, preset, occ):
    """The failing call and a good one queued behind it before the flush, which must apply nothing; then
    values, the error triple and the closed store against the oracle, clear_error, and a further call."""
    kt = len(name) % 2 if "key-" not in name else 1  # 4-byte keys compare as 64-bit values here (header)
    case, st = MAT(kt, W, 40), torch.cuda.Stream()
    init = np.full((40, W), 5, np.int32)
    for r, c_, x in preset:
        init[r, c_] = x
    s, o = pair(case, oracle, np.full((40, W), 5, np.int32))
    try:
        s.readAll(init.astype(">i4").tobytes())  # unchecked, like the reference's readAll
        assert o.read_all(init.astype(">i4").tobytes()) == 0
        keys, c, v = (np.array([[q[i]] for q in occ]) for i in range(3))
        keys, c, v = case["first"] + keys[:, 0].astype(np.int64), c.astype(np.int32), v.astype(np.int32)
        good = (case["first"] + np.array([0, 7], np.int64), np.array([[0], [W - 1]], np.int32), np.ones((2, 1), np.int32))
        co.set_long_min(lmin)
        keep = push(s, co, keys, c, v, 4, st.cuda_stream)
        rc = o.push(host_push(case, keys, c, v))
        assert (rc != 0) == (name != "dip-ends-nonnegative")
        if rc:
            with pytest.raises(DistMLException) as e:  # from the flush, or from the queued call's entry
                keep += push(s, co, *good, 12, st.cuda_stream)
                s.flush()
            assert (e.value.code, e.value.key, e.value.col) == o.error()
            assert state(s) == ostate(o)
            with pytest.raises(DistMLException):
                push(s, co, *good)
            s.clear_error(), o.clear_error()
            assert state(s) == ostate(o)
        else:
            keep += push(s, co, *good, 12, st.cuda_stream)
            s.flush()
        assert o.push(host_push(case, *good)) == 0
        rc and push(s, co, *good)  # the dip's queued call was applied; after a failure it was not
        assert state(s) == ostate(o)
    finally:
        co.set_long_min(0)
        s.close()


@pytest.mark.parametrize("per", [1, 4])
def test_int_array_store(co, oracle, per):
    """n = 1 ... 3 000 with one key holding most of the list, either key width; then a call whose lowest
    key goes negative: the later keys' adds are taken back and the error has no column."""
    case, rng = ARR(per % 2), np.random.default_rng(per)
    s, o = pair(case, oracle, rng.integers(2 ** 29, 2 ** 30, size=(ROWS, 1)).astype(np.int32))
    try:
        for i, n in enumerate([1, 63, 64, 65, 3000]):
            keys = case["first"] + np.where(rng.random(n) < 0.7, 17, rng.integers(0, ROWS, size=n)).astype(np.int64)
            v = rng.integers(-2 ** 18, 2 ** 18, size=(n, per)).astype(np.int32)
            keep = push(s, co, keys, None, v, (4, 12)[i % 2])
            assert o.push(host_push(case, keys, None, v)) == 0 and state(s) == ostate(o), n
            [a.check() for a in keep]
        keys, v = case["first"] + np.array([9, 300, 9, 2, 2], np.int64), np.full((5, per), -2 ** 29 // per, np.int32)  # -2^30 per key
        v[1] = 1
        with pytest.raises(DistMLException) as e:
            push(s, co, keys, None, v)
        assert o.push(host_push(case, keys, None, v)) != 0
        assert (e.value.code, e.value.key, e.value.col) == o.error() == (_lib.DML_E_NEGATIVE_COUNTER, case["first"] + 2, -1)
        assert state(s) == ostate(o)
    finally:
        s.close()


def test_refusals(co, oracle):
    """Every refusal of the header, with stores, coalescer and inputs unchanged; n == 0 is DML_OK."""
    from distml_amd import Coalescer
    L, vp = _lib.load(), lambda x: C.c_void_p(x or None)  # noqa: E731
    mat, arr = MAT(1, 5), ARR(0)
    others = [fc._case("f32", 1, 0, 1, 5, ROWS, 1000), fc._case("ada", 1, 1, 1, 5, ROWS, 1000, True), fc._case("af32", 0, 0, 1, 1, ROWS, 1000)]
    (s, o), (a, _) = (pair(x, oracle, np.full((ROWS, x["cols"]), 2 ** 29, np.int32)) for x in (mat, arr))
    floats = [make_store(x, fc.build_init(x, plain=True)) for x in others]
    try:
        keys, c, v = shard_moves(mat, 9, 2, seed=3)
        ka, ca, va = (geom.pack([x.tobytes()], 4 if i else 0) for i, x in enumerate((keys, c, v)))
        k, cp, vv, h, ch = ka.ptrs[0], ca.ptrs[0], va.ptrs[0], s._h, co._h
        before = [x.values().tobytes() for x in [s, a] + floats]
        bad = [("null store", (None, ch, k, 9, 2, cp, vv)), ("null coalescer", (h, None, k, 9, 2, cp, vv)),
               ("n < 0", (h, ch, k, -1, 2, cp, vv)), ("n = 2^31", (h, ch, k, 1 << 31, 2, cp, vv)),
               ("per_occ 0", (h, ch, k, 9, 0, cp, vv)), ("per_occ 17", (h, ch, k, 9, 17, cp, vv)),
               ("null keys", (h, ch, 0, 9, 2, cp, vv)), ("null cols", (h, ch, k, 9, 2, 0, vv)), ("null vals", (h, ch, k, 9, 2, cp, 0)),
               ("keys + 4", (h, ch, k + 4, 8, 2, cp, vv)), ("cols + 2", (h, ch, k, 9, 2, cp + 2, vv)),
               ("vals + 2", (h, ch, k, 9, 2, cp, vv + 2)), ("array with cols", (a._h, ch, k, 9, 2, cp, vv))]
        other = Coalescer(1) if torch.cuda.device_count() > 1 else None
        other and bad.append(("coalescer of another device", (h, other._h, k, 9, 2, cp, vv)))
        for what, (hh, cc, kk, n, per, cq, vq) in bad:
            assert L.dml_store_push_elems_device(hh, cc, vp(kk), n, per, vp(cq), vp(vq), None) == _lib.DML_E_INVALID_ARG, what
        for x in floats:
            assert L.dml_store_push_elems_device(x._h, ch, vp(k), 9, 2, vp(cp), vp(vv), None) == _lib.DML_E_UNSUPPORTED
        assert L.dml_store_push_elems_device(h, ch, None, 0, 2, None, None, None) == 0
        assert [x.values().tobytes() for x in [s, a] + floats] == before
        assert all(x.error_state()[0] == 0 for x in [s, a] + floats)
        [x.check() for x in (ka, ca, va)]
        push(s, co, keys, c, v)  # the coalescer and the store still work
        assert o.push(host_push(mat, keys, c, v)) == 0 and state(s) == ostate(o)
        other and other.close()
    finally:
        [x.close() for x in [s, a] + floats]

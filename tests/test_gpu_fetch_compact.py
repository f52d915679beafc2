"""The compact fetch's two endpoints against plain numpy: np.nonzero of the expected rows
for dml_store_fetch_compact_rows_device, np.add.at on zeroed rows for dml_compact_rows_expand_device.
Every output sits in geom.OutArena poison; what a call must not write must still be poison."""
from contextlib import closing

import numpy as np
import pytest

import fetch_cases as fc
import geom
from distml_amd import (ArrayIndexOutOfBoundsException, Coalescer, DeviceKeys, NativeError, _lib, encode_matrix_push,
                        expand_compact_rows_device)
from test_gpu_worker_iteration import _gpu, make_store  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# 1 - 3 dwords; whole and ragged vectors; one round's edge (64 lanes); one slice's edge; two and three slices
COLS = (1, 3, 4, 5, 63, 64, 65, 1000, 1024, 1025, 2049)
ROWS, INT_MIN, POISON = 40, -(1 << 31), geom.poison_i32()


def case_of(cols, rows=ROWS):  # 4- and 8-byte-key descs alternate down COLS
    return fc._case("i32", 1, cols % 2, 0, cols, rows, geom.BIG33 if cols % 2 else geom.NEG32)


def contents(cols, density, rows=ROWS):
    rng = np.random.default_rng(cols * 3 + len(density))
    a = rng.integers(INT_MIN, 1 << 31, size=(rows, cols)).astype(np.int32)
    a[a == 0] = 1
    a.flat[::3], a.flat[1::7] = -1, INT_MIN
    a *= density != "zero"
    if density == "sparse":
        a[rng.random((rows, cols)) >= 0.05] = 0
        a[1], a[2] = 0, 0
        a[1, cols - 1], a[2, 0] = INT_MIN, -1  # only the last column; only column 0
    return a


def store_of(case, a):
    s = make_store(case, np.zeros_like(a))
    s.readAll(a.astype(">i4").tobytes())  # negative counters arrive the way a checkpoint brings them
    return s


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dt).copy()).cuda()


def keys_of(case, seed, n):  # descending, then repeats in any order
    r = np.concatenate([np.arange(case["rows"])[::-1], np.random.default_rng(seed).integers(0, case["rows"], size=n)])
    return case["first"] + r[:n].astype(np.int64)


def compact(rows):  # (ptr, ecol, eval) of dense int32 rows
    r, c = np.nonzero(rows)
    return np.concatenate([[0], np.cumsum((rows != 0).sum(1))]).astype(np.int32), c.astype(np.int32), rows[r, c]


class Out:  # ptr, ecol and eval of one fetch of n keys with room for cap entries, at 4, 8 and 12 mod 16
    def __init__(self, n, cap):
        self.a = [geom.OutArena(b, lead).upload() for b, lead in (((n + 1) * 4, 4), (cap * 4, 8), (cap * 4, 12))]
        self.n, self.cap = n, cap

    def fetch(self, s, dk, stream=None, want=False):
        torch.cuda.synchronize()
        ec, ev = (x.ptr if self.cap else None for x in self.a[1:])  # cap 0: the count-only call, null entry arrays
        return s.handleFetchCompactRowsDevice(s.format, DeviceKeys(dk.data_ptr(), self.n), self.a[0].ptr, ec, ev,
                                              self.cap, stream, want)

    def check(self, want, written=True):  # ptr whole; the entries, or nothing `written`; every other byte is poison
        for x, w in zip(self.a, [want[0].tobytes()] + [w.tobytes() if written else b"" for w in want[1:]]):
            assert x.read().tobytes()[:len(w)] == w
            x.untouched([(0, len(w))])


@pytest.mark.parametrize("density", ["zero", "full", "sparse"])
@pytest.mark.parametrize("cols,rows,n", [(c, ROWS, 53) for c in COLS] + [(8, 500, 4100)])  # 4100: k_cr_scan carries
def test_fetch_bytes(cols, rows, n, density):
    case, a = case_of(cols, rows), contents(cols, density, rows)
    keys = keys_of(case, n + cols, n)
    want = compact(a[keys - case["first"]])
    with closing(store_of(case, a)) as s:
        dk = dev(keys, np.int64)
        for spare in (3, 0):  # two calls, both numpy's bytes and so each other's; the second with cap_entries == nnz
            o = Out(n, len(want[1]) + spare)
            assert o.fetch(s, dk, want=True) == len(want[1]) == want[0][-1]
            o.check(want)
        assert s.error_state()[0] == 0


@pytest.mark.parametrize("cols", [4, 1025])
def test_refused_keys(cols):
    """An alias 2^32 above an in-shard key, first - 1 and last + 1: empty ranges, every other row as expected; the
    error names the key at the lowest bad index, from the synchronous call and from flush() behind a stream."""
    case, a = case_of(cols), contents(cols, "sparse")
    first, keys, good = case["first"], keys_of(case, cols, 30), np.ones(30, bool)
    keys[[4, 11, 29]], good[[4, 11, 29]] = (first + 3 + geom.ALIAS, first - 1, first + ROWS), False
    want = compact(np.where(good[:, None], a[np.where(good, keys - first, 0)], 0))
    E, dk, st = (_lib.DML_E_KEY_OUT_OF_SHARD, int(keys[4]), -1), dev(keys, np.int64), torch.cuda.Stream()
    with closing(store_of(case, a)) as s:
        for stream in (None, st.cuda_stream):
            o = Out(30, len(want[1]))
            with pytest.raises(ArrayIndexOutOfBoundsException) as e:
                o.fetch(s, dk, stream=stream)
                s.flush()
            assert (e.value.code, e.value.key, e.value.col) == E and s.error_state() == E
            o.check(want)
            s.clear_error()


def test_capacity():
    case, a, keys = case_of(1025), contents(1025, "sparse"), keys_of(case_of(1025), 5, 53)
    want, dk, st = compact(a[keys - case["first"]]), dev(keys, np.int64), torch.cuda.Stream()
    with closing(store_of(case, a)) as s:
        o = Out(53, len(want[1]) - 1)  # cap_entries == nnz succeeds: test_fetch_bytes' second call
        with pytest.raises(NativeError) as e:
            o.fetch(s, dk, stream=st.cuda_stream, want=True)
        assert e.value.code == _lib.DML_E_CAPACITY
        o.check(want, written=False)  # ptr whole, ptr[n] == nnz; no entry stored
        o = Out(53, 0)  # the count-only call: the caller reads ptr[n]
        assert o.fetch(s, dk) is None and s.error_state()[0] == 0
        o.check(want, written=False)


def test_ordering_between_pushes():
    """pushDevice A, compact fetch on a torch stream, pushDevice B, no flush: the list is the state after A alone."""
    case, rng = case_of(1000), np.random.default_rng(78)
    init, asc = contents(1000, "zero"), case["first"] + np.arange(ROWS, dtype=np.int64)
    A, B = (encode_matrix_push(asc, rng.integers(0, 2, size=(ROWS, 1000)).astype(np.int32), 0, 0) for _ in "AB")
    with closing(make_store(case, init)) as s, closing(make_store(case, init)) as twin:
        twin.handlePush(twin.format, A)
        keys = keys_of(case, 78, 90)
        want = compact(np.asarray(twin.values()).reshape(ROWS, -1)[keys - case["first"]])
        pa, pb, dk, o, st = geom.pack([A], 4), geom.pack([B], 4), dev(keys, np.int64), Out(90, len(want[1])), torch.cuda.Stream()
        s.pushDevice(pa.ptrs, pa.lens)
        o.fetch(s, dk, stream=st.cuda_stream)
        s.pushDevice(pb.ptrs, pb.lens)
        o.check(want)
        twin.handlePush(twin.format, B)
        assert s.values().tobytes() == twin.values().tobytes()


def expand(ptr, ecol, ev, entries, cols, inv, n):  # (the device's plane, numpy's), poison where a row stays untouched
    m, plane = len(ptr) - 1, geom.OutArena(n * cols * 4, 4).upload()
    d = [dev(x) for x in (ptr, ecol, ev, [] if inv is None else inv)]
    expand_compact_rows_device(*(x.data_ptr() for x in d[:3]), m, entries, cols, d[3].data_ptr(), n, plane.ptr)
    want = np.full((n, cols), POISON, np.int32)
    for j, u in enumerate(range(n) if inv is None else inv):
        if 0 <= u < m and 0 <= ptr[u] <= ptr[u + 1] <= entries:
            c, v = ecol[ptr[u]:ptr[u + 1]], ev[ptr[u]:ptr[u + 1]]
            ok, row = (c >= 0) & (c < cols), np.zeros(cols, np.uint32)
            np.add.at(row, c[ok], v[ok].view(np.uint32))
            want[j] = row.view(np.int32)
    got = plane.read().view(np.int32).reshape(n, cols).copy()
    plane.untouched([(0, plane.nbytes)])
    return got, want


@pytest.mark.parametrize("m", [1, 9, 70])
@pytest.mark.parametrize("cols", COLS)
def test_expand(cols, m):
    rng = np.random.default_rng(cols + m)
    ptr, ecol, ev = compact(contents(cols, "sparse" if m > 1 else "full", m))
    E, inv = len(ecol), rng.integers(0, m, size=2 * m + 3).astype(np.int32)  # repeats
    inv[[0, m]] = -1, m  # both rows keep their fill pattern
    (canonical, want), (got, same) = expand(ptr, ecol, ev, E, cols, inv, len(inv)), expand(ptr, ecol, ev, E, cols, None, m)
    assert canonical.tobytes() == want.tobytes() and got.tobytes() == same.tobytes()
    # the same rows, not canonical: every entry split into two summands, columns -1 and cols beside them, shuffled
    rows = []
    for u in range(m):
        c, v = ecol[ptr[u]:ptr[u + 1]], ev[ptr[u]:ptr[u + 1]].view(np.uint32)
        part, p = rng.integers(0, 1 << 32, size=len(c), dtype=np.uint64).astype(np.uint32), rng.permutation(2 * len(c) + 2)
        rows.append((np.concatenate([c, c, [-1, cols]])[p], np.concatenate([part, v - part, [7, 9]])[p]))
    ptr2 = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int32)
    ecol2, ev2 = (np.concatenate([r[i] for r in rows]).astype(np.uint32).view(np.int32) for i in (0, 1))
    got, _ = expand(ptr2, ecol2, ev2, len(ecol2), cols, inv, len(inv))
    assert got.tobytes() == canonical.tobytes()
    # rows m (ptr[u] > ptr[u + 1]) and m + 2 (ptr[u + 1] > entries) are left untouched; row m + 1 between them is whole
    got, want = expand(np.concatenate([ptr, [E - 1, E, E + 5]]).astype(np.int32), ecol, ev, E, cols, None, m + 3)
    assert got.tobytes() == want.tobytes() and (got[[m, m + 2]] == POISON).all()


@pytest.mark.parametrize("cols", [1000, 2049])
def test_round_trip(cols):
    """Coalescer.run (keys only) -> compact fetch of the distinct keys -> expand by the inverse == the plane fetch."""
    case, a, keys = case_of(cols), contents(cols, "sparse"), keys_of(case_of(cols), cols, 100)
    with closing(store_of(case, a)) as s, closing(Coalescer(0)) as co:
        dk, uk, inv = dev(keys, np.int64), dev(np.zeros(100), np.int64), dev(np.zeros(100))
        m = co.run(s.format, cols, DeviceKeys(dk.data_ptr(), 100), None, uk.data_ptr(), None, inv.data_ptr(), 100)
        o = Out(m, m * cols)
        E = o.fetch(s, uk, want=True)
        planes = [geom.OutArena(100 * cols * 4, 4).upload() for _ in "ab"]
        expand_compact_rows_device(*(x.ptr for x in o.a), m, E, cols, inv.data_ptr(), 100, planes[0].ptr)
        s.handleFetchPlanesDevice(s.format, DeviceKeys(dk.data_ptr(), 100), planes[1].ptr)
        assert planes[0].read().tobytes() == planes[1].read().tobytes() == a[keys - case["first"]].tobytes()


K, P, C, V = (0x10000000 + i * 0x100000 for i in range(4))
REFUSED = [("n-negative", dict(n=-1)), ("n-2^31", dict(n=1 << 31)), ("cap-negative", dict(cap=-1)),
           ("keys-null", dict(k=0)), ("ptr-null", dict(p=0)), ("ecol-null", dict(c=0)), ("eval-null", dict(v=0)),
           ("keys-misaligned", dict(k=K + 4)), ("ptr-misaligned", dict(p=P + 2)), ("eval-misaligned", dict(v=V + 1)),
           ("ptr-over-keys", dict(p=K + 8 * 9 - 4)), ("ecol-over-ptr", dict(c=P + 4 * 9)), ("eval-over-ecol", dict(v=C + 4)),
           ("f32", fc._case("f32", 1, 0, 1, 5, ROWS, 1000)), ("ada", fc._case("ada", 1, 0, 1, 5, ROWS, 1000, True)),
           ("f64", fc._case("f64", 1, 1, 3, 5, ROWS, 1000)), ("ai32", fc._case("ai32", 0, 0, 0, 1, ROWS, 1000))]


@pytest.mark.parametrize("what,over", REFUSED, ids=[w for w, _ in REFUSED])
def test_refusals(what, over):
    """Made-up addresses no kernel may see; `over` a case: a store that is not an IntMatrixStore. Nothing changes."""
    other, a = "id" in over, contents(5, "sparse")
    with closing(make_store(over, fc.build_init(over)) if other else store_of(case_of(5), a)) as s:
        g = {**dict(k=K, n=9, p=P, c=C, v=V, cap=45), **({} if other else over)}
        rc = _lib.load().dml_store_fetch_compact_rows_device(s._h, g["k"] or None, g["n"], g["p"] or None, g["c"] or None,
                                                             g["v"] or None, g["cap"], None, None)
        assert rc == (_lib.DML_E_UNSUPPORTED if other else _lib.DML_E_INVALID_ARG) and s.error_state()[0] == 0
        assert s.values().tobytes() == (fc.build_init(over) if other else a).tobytes()

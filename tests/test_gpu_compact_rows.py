"""Compact update rows: dml_coalesce_elems_compact_device (Coalescer.run_elems_compact), dml_compact_rows_split
and dml_store_push_compact_rows_device (DataStore.handlePushCompactRowsDevice). The expected rows are np.add.at
into int64 wrapped to int32; the expected store is the CPU oracle fed one push of those dense records. Every
comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom
from test_gpu_coalesce_elems import NEVER, _gpu, co, expect, fmt, moves  # noqa: F401  (_gpu: the GPU gate)
from test_gpu_push_elems import ostate, pair, state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from distml_amd import DeviceKeys, KeyRange, _lib, compact_rows_split, encode_matrix_push  # noqa: E402

COLS, W, BIG33 = [1, 3, 1000, 1030], 1030, geom.BIG33
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731


def elems(cols, per, seed, first=0, shift=0, lone=0):
    """A seeded element list over keys first + 0 .. 8 (+ `lone` single-occurrence keys behind them), shuffled:
    segments of 7, 8 and 200 occurrences (the last spread over every column: more than 64 non-zeros in a
    slice), 64, 65 and 1; a key whose two deltas cancel; a key whose columns all lie outside the row; a key of
    65 x 2^30 on one column (the sum wraps). Deltas are drawn below 2^30 and shifted right by `shift`."""
    rng = np.random.default_rng(seed)
    seg = [7, 8, 200, 64, 65, 1, 2, 3, 65] + [1] * lone
    keys = first + np.repeat(np.arange(len(seg)), seg).astype(np.int64)
    n, at = len(keys), np.concatenate([[0], np.cumsum(seg)])
    c = rng.integers(0, cols, size=(n, per)).astype(np.int32)
    v = (rng.integers(-2 ** 30, 2 ** 30, size=(n, per)) >> shift).astype(np.int32)
    v[v == 0] = 1
    c[at[6]:at[7]], v[at[6]], v[at[6] + 1] = cols - 1, 5, -5
    c[at[7]:at[8]] = np.array([-1, cols, 2 ** 31 - 1])[:, None]
    c[at[8]:at[9]], v[at[8]:at[9]] = cols // 2, 2 ** 30 >> shift
    p = rng.permutation(n)
    return keys[p], c[p], v[p]


def compact(keys, c, v, cols):
    """(distinct keys, inverse, dense rows, ptr, ecol, eval) by numpy."""
    uk, inv, plane, _ = expect(keys, c, v, cols, 1, False)
    rows = np.frombuffer(plane, np.int32).reshape(len(uk), cols)
    r, cc = np.nonzero(rows)
    ptr = np.concatenate([[0], np.cumsum((rows != 0).sum(axis=1))]).astype(np.int32)
    return uk, inv, rows, ptr, cc.astype(np.int32), rows[r, cc]


def run_compact(co, cols, per, keys, c, v, cap_rows, cap_entries, want=False):
    """One source call into poisoned outputs; returns (rc, m, nnz, [keys, ptr, ecol, eval, inverse] arenas)."""
    n = len(keys)
    ins = [dev(keys), dev(c), dev(v)]
    outs = [geom.OutArena(max(cap_rows, 1) * 8, 8).upload(), geom.OutArena((max(cap_rows, 0) + 1) * 4, 4).upload(),
            geom.OutArena(max(cap_entries, 1) * 4, 12).upload(), geom.OutArena(max(cap_entries, 1) * 4, 4).upload(),
            geom.OutArena(n * 4, 12).upload()]
    m, nnz = C.c_int64(-7), C.c_int64(-7)
    rc = _lib.load().dml_coalesce_elems_compact_device(
        co._h, C.byref(fmt(1).to_c()), cols, ins[0].data_ptr(), n, per, ins[1].data_ptr(), ins[2].data_ptr(), outs[0].ptr,
        outs[1].ptr, outs[2].ptr, outs[3].ptr, cap_rows, cap_entries, outs[4].ptr, C.byref(m), C.byref(nnz) if want else None, None)
    return rc, m.value, nnz.value, outs


@pytest.mark.parametrize("per", [1, 2, 16])
@pytest.mark.parametrize("cols", COLS)
def test_source(co, cols, per):
    """The four arrays and the inverse against numpy on both sides of long_min 8 (keys of 7, 8 and 200), twice on the
    long side (two runs, equal bytes), m = BLOCK_KEYS + 3 at per 2, and one-key lists of 1, 64 and 65 occurrences."""
    lists = [elems(cols, per, cols + per, -4, lone=(_lib.DML_COALESCE_BLOCK_KEYS - 6) * (per == 2))]
    lists += [moves(n, cols, per, cols + per + n) for n in (1, 64, 65)]
    try:
        for keys, c, v in lists:
            uk, inv, _, ptr, ecol, ev = compact(keys, c, v, cols)
            n, m, nnz = len(keys), len(uk), len(ecol)
            for thr in (NEVER, 8, 8):
                co.set_long_min(thr)
                rc, gm, gn, outs = run_compact(co, cols, per, keys, c, v, m, n * per, want=True)
                assert (rc, gm, gn) == (0, m, nnz), (n, thr)
                for a, b in zip(outs, (uk, ptr, ecol, ev, inv)):
                    assert a.read()[:b.nbytes].tobytes() == b.tobytes(), (n, thr)
                    a.untouched([(0, b.nbytes)])
            ko, io = geom.OutArena(m * 8, 8).upload(), geom.OutArena(n * 4, 4).upload()  # the dense call's keys and inverse
            plane = torch.empty((m, cols), dtype=torch.int32, device="cuda")
            k, cc, vv = dev(keys), dev(c), dev(v)
            co.run_elems(fmt(1), cols, DeviceKeys(k.data_ptr(), n), cc.data_ptr(), vv.data_ptr(), per, plane.data_ptr(), m * cols * 4,
                         False, ko.ptr, io.ptr)
            assert ko.read().tobytes() == outs[0].read()[:m * 8].tobytes() and io.read().tobytes() == outs[4].read().tobytes()
    finally:
        co.set_long_min(0)


@pytest.mark.parametrize("short", ["rows", "entries"])
def test_source_capacity(co, short):
    """One row, or one entry under min(n x per_occ, m x cols), short: DML_E_CAPACITY, m reported, no byte written."""
    keys, c, v = elems(1000, 2, 5)
    m, bound = 9, min(len(keys) * 2, 9 * 1000)
    rc, gm, _, outs = run_compact(co, 1000, 2, keys, c, v, m - (short == "rows"), bound - (short == "entries"))
    assert (rc, gm) == (_lib.DML_E_CAPACITY, m)
    for a in outs:
        a.read()
        a.untouched([])


def push(s, uk, ptr, ecol, ev, stream=None):
    t = [dev(uk), dev(ptr), dev(np.append(ecol, 0).astype(np.int32)), dev(np.append(ev, 0).astype(np.int32))]
    s.handlePushCompactRowsDevice(s.format, DeviceKeys(t[0].data_ptr(), len(uk)), *(x.data_ptr() for x in t[1:]), stream=stream)
    return t  # alive until the apply stream has passed the call


@pytest.mark.parametrize("kt", [0, 1], ids=["k4", "k8"])
@pytest.mark.parametrize("cols", COLS)
def test_owner_parity(co, oracle, cols, kt):
    """The source test's list into a store on a side stream, then a plane fetch with no flush, which must see it."""
    case, st = fc._case("i32", 1, kt, 0, cols, 12, (geom.NEG32, BIG33)[kt]), torch.cuda.Stream()
    rng = np.random.default_rng(cols)
    s, o = pair(case, oracle, rng.integers(2 ** 29, 2 ** 30, size=(12, cols)).astype(np.int32))
    try:
        uk, _, rows, ptr, ecol, ev = compact(*elems(cols, 2, cols, case["first"], shift=12), cols)
        got, fk = torch.empty((9, cols), dtype=torch.int32, device="cuda"), dev(uk)
        keep = push(s, uk, ptr, ecol, ev, st.cuda_stream)
        s.handleFetchPlanesDevice(s.format, DeviceKeys(fk.data_ptr(), 9), got.data_ptr(), None, stream=st.cuda_stream)
        assert o.push(encode_matrix_push(uk, rows, kt, 0)) == 0
        st.synchronize()
        assert got.cpu().numpy().tobytes() == o.data[:9].tobytes()
        s.flush()
        assert state(s) == ostate(o) and keep
    finally:
        s.close()


# (id, counters preset as (row, col, value), [(row, [(col, value), ...])] ascending); every other counter starts
# at 5. Rows are shard rows of a 40-row store of W = 1030 columns: row 40 is last + 1 and row -1 is first - 1.
VERDICTS = [
    ("second-slice-of-middle-key", [], [(3, [(0, 1)]), (7, [(2, 1), (1026, -6), (1029, 1)]), (9, [(1, 1)])]),
    ("empty-range-over-negative", [(6, 9, -3)], [(5, [(0, 1)]), (6, []), (8, [(1, 1)])]),
    ("key-below-first", [], [(-1, [(0, 1)]), (5, [(1, 1)])]),
    ("key-above-last", [], [(5, [(1, 1)]), (39, [(1029, 1)]), (40, [(0, 1)]), (41, [(1, 1)])]),
    ("below-first-and-negative", [], [(-1, [(0, 1)]), (5, [(1, -6)])]),
    ("above-last-and-negative", [], [(5, [(1, -6)]), (6, [(0, 1)]), (40, [(0, 1)])]),
    ("not-canonical", [], [(4, [(7, 2), (3, 1), (7, 3), (-1, 9), (1030, 9), (3, -1)]), (5, [])]),
    ("block-route-fails", [], [(2, [(1, 1)]), (4, [(i % W, 1 - 7 * (i == 1027)) for i in range(1100)]), (6, [(0, 1)])]),
]


@pytest.mark.parametrize("name,preset,lst", VERDICTS, ids=[v[0] for v in VERDICTS])
def test_owner_verdicts(co, oracle, name, preset, lst):
    """The call and a good one queued behind it before the flush (applied only if the first closed nothing); values,
    the error triple and the closed store against the oracle's push of the dense records."""
    kt = 1
    case, st = fc._case("i32", 1, kt, 0, W, 40, BIG33), torch.cuda.Stream()
    init = np.full((40, W), 5, np.int32)
    for r, c_, x in preset:
        init[r, c_] = x
    s, o = pair(case, oracle, np.full((40, W), 5, np.int32))
    try:
        s.readAll(init.astype(">i4").tobytes())  # unchecked, like the reference's readAll
        assert o.read_all(init.astype(">i4").tobytes()) == 0
        uk = case["first"] + np.array([r for r, _ in lst], np.int64)
        ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in lst])]).astype(np.int32)
        ent = np.array([cv for _, e in lst for cv in e], np.int64).reshape(-1, 2)
        dense = np.zeros((len(lst), W), np.int64)
        ok = (ent[:, 0] >= 0) & (ent[:, 0] < W)
        np.add.at(dense, (np.repeat(np.arange(len(lst)), np.diff(ptr))[ok], ent[ok, 0]), ent[ok, 1])
        good = (case["first"] + np.array([0, 7], np.int64), np.array([0, 1, 2], np.int32), np.array([0, W - 1], np.int32), np.ones(2, np.int32))
        keep = push(s, uk, ptr, ent[:, 0].astype(np.int32), ent[:, 1].astype(np.int32), st.cuda_stream)
        rc = o.push(encode_matrix_push(uk, dense.astype(np.int32), kt, 0))
        assert (rc != 0) == (name != "not-canonical")
        if rc:
            with pytest.raises(Exception):  # from the flush, or from the queued call's entry
                keep += push(s, *good, st.cuda_stream)
                s.flush()
            assert s.error_state() == o.error() and state(s) == ostate(o)
            s.clear_error(), o.clear_error()
        else:
            keep += push(s, *good, st.cuda_stream)
            s.flush()
            gd = np.zeros((2, W), np.int32)
            gd[0, 0] = gd[1, W - 1] = 1
            assert o.push(encode_matrix_push(good[0], gd, kt, 0)) == 0
        assert state(s) == ostate(o)
    finally:
        s.close()


@pytest.mark.parametrize("name,keys,ptr,bad", [("keys-not-ascending", [3, 9, 9, 12], [0, 1, 2, 3, 4], 9),
                                              ("ptr-decreasing", [3, 9, 10, 12], [0, 2, 1, 3, 4], -1),
                                              ("ptr0-not-zero", [3, 9, 10, 12], [1, 1, 2, 3, 4], -1)])
def test_owner_malformed(co, oracle, name, keys, ptr, bad):
    """A malformed list applies nothing and closes the store with (DML_E_INVALID_ARG, key or -1, -1)."""
    case = fc._case("i32", 1, 1, 0, 3, 40, BIG33)
    s, o = pair(case, oracle, np.full((40, 3), 5, np.int32))
    try:
        uk = case["first"] + np.array(keys, np.int64)
        with pytest.raises(Exception):
            push(s, uk, np.array(ptr, np.int32), np.zeros(4, np.int32), np.ones(4, np.int32))
        assert s.error_state() == (_lib.DML_E_INVALID_ARG, case["first"] + bad if bad >= 0 else -1, -1)
        assert s.values().tobytes() == o.data.tobytes()
    finally:
        s.close()


def test_split_end_to_end(co, oracle):
    """run_elems_compact over the keys of a 2-way linearSplit plus -1 and total_rows, the split, each run into its
    own store: both shards equal the oracle's stores fed the dense records of their keys; the dropped keys reach neither."""
    total, cols, per = 21, 1030, 2
    keys, c, v = elems(cols, per, 11, -1, shift=12, lone=14)  # keys -1 .. 21
    uk, _, rows, _, _, _ = compact(keys, c, v, cols)
    n, m = len(keys), len(uk)
    k, cc, vv = dev(keys), dev(c), dev(v)
    ko, po = torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m + 1, dtype=torch.int32, device="cuda")
    eo = torch.empty((2, n * per), dtype=torch.int32, device="cuda")
    assert co.run_elems_compact(fmt(1), cols, DeviceKeys(k.data_ptr(), n), cc.data_ptr(), vv.data_ptr(), per, ko.data_ptr(),
                                po.data_ptr(), eo[0].data_ptr(), eo[1].data_ptr(), m, n * per)[0] == m
    off, p2 = torch.empty((2, 3), dtype=torch.int64, device="cuda"), torch.empty(m + 2, dtype=torch.int32, device="cuda")
    compact_rows_split(DeviceKeys(ko.data_ptr(), m), po.data_ptr(), total, 2, off[0].data_ptr(), off[1].data_ptr(), p2.data_ptr())
    ro, eoff = off.cpu().numpy().tolist()
    assert ro == [1, 1 + 11, 1 + 21]  # step 11: owner 0 holds keys 0 .. 10, owner 1 keys 11 .. 20
    for q, r in enumerate(KeyRange(0, total - 1).linearSplit(2)):
        case = fc._case("i32", 1, 1, 0, cols, r.lastKey - r.firstKey + 1, r.firstKey)
        s, o = pair(case, oracle, np.full((case["rows"], cols), 2 ** 29, np.int32))
        try:
            s.handlePushCompactRowsDevice(s.format, DeviceKeys(ko.data_ptr() + 8 * ro[q], ro[q + 1] - ro[q]), p2.data_ptr() + 4 * (ro[q] + q),
                                          eo[0].data_ptr() + 4 * eoff[q], eo[1].data_ptr() + 4 * eoff[q])
            assert o.push(encode_matrix_push(uk[ro[q]:ro[q + 1]], rows[ro[q]:ro[q + 1]], 1, 0)) == 0 and state(s) == ostate(o)
        finally:
            s.close()

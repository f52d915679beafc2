"""dml_store_push_compact_rows_batch_device (DataStore.handlePushCompactRowsBatchDevice): R compact row lists in
one pass over the shard. The expected store is the CPU oracle fed one record push of the dense rows per run, in
order, stopping at the first push it refuses. Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom
from test_gpu_coalesce_elems import _gpu, co  # noqa: F401  (_gpu: the GPU gate)
from test_gpu_compact_rows import BIG33, W, compact, dev, elems, push
from test_gpu_push_elems import ostate, pair, state
from test_gpu_worker_iteration import make_store

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from distml_amd import DeviceKeys, _lib, encode_matrix_push  # noqa: E402


def upload(lists):
    """[(keys, ptr, ecol, eval)] -> (the call's runs, the tensors, alive until the apply stream has passed the call)."""
    keep = [[dev(k), dev(p), dev(np.append(c, 0).astype(np.int32)), dev(np.append(v, 0).astype(np.int32))] if len(k) else None
            for k, p, c, v in lists]
    runs = [(DeviceKeys(t[0].data_ptr(), len(t[0])), *(x.data_ptr() for x in t[1:])) if t else (DeviceKeys(0, 0), None, None, None)
            for t in keep]
    return runs, keep


def raw(first, lst, cols=W):
    """A run written as [(shard row, [(col, value), ...])]: (keys, ptr, ecol, eval, dense rows), taken as it is."""
    keys = first + np.array([r for r, _ in lst], np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(e) for _, e in lst])]).astype(np.int32)
    ent = np.array([cv for _, e in lst for cv in e], np.int64).reshape(-1, 2)
    dense, ok = np.zeros((len(lst), cols), np.int64), (ent[:, 0] >= 0) & (ent[:, 0] < cols)
    np.add.at(dense, (np.repeat(np.arange(len(lst)), np.diff(ptr))[ok], ent[ok, 0]), ent[ok, 1])
    return keys, ptr, ent[:, 0].astype(np.int32), ent[:, 1].astype(np.int32), dense.astype(np.int32)


def feed(o, kt, runs):
    """One record push per non-empty run of (keys, ..., dense), in order, up to the first the oracle refuses."""
    for r in runs:
        if len(r[0]) and o.push(encode_matrix_push(r[0], r[-1], kt, 0)):
            return True
    return False


@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("kt", [0, 1], ids=["k4", "k8"])
@pytest.mark.parametrize("cols", [1, 3, 1000, 1030])
def test_parity(co, oracle, cols, kt, R):
    """Keys 0 .. 8 in every run (two of them with an empty entry range), key 9 only in the first run, 10 only in a
    middle one, 11 only in the last, run 1 of m == 0 (R > 1). A side stream, then a plane fetch with no flush."""
    case, st = fc._case("i32", 1, kt, 0, cols, 12, (geom.NEG32, BIG33)[kt]), torch.cuda.Stream()
    s, o = pair(case, oracle, np.random.default_rng(cols).integers(2 ** 29, 2 ** 30, size=(12, cols)).astype(np.int32))
    both = cols == 1030 and kt == 1 and R == 3  # one parameter set: a second store fed by R single calls
    s2 = make_store(case, o.data.copy()) if both else None
    try:
        lists = []
        for q in range(R):
            keys, c, v = elems(cols, 2, 7 * cols + q, case["first"], shift=12, lone=3)
            own = list(range(9)) + [9] * (q == 0) + [10] * (q == R // 2) + [11] * (q == R - 1)
            sel = np.isin(keys - case["first"], own) & (q != 1 or R == 1)
            uk, _, rows, ptr, ecol, ev = compact(keys[sel], c[sel], v[sel], cols) if sel.any() else (np.zeros(0, np.int64),) + (None,) * 5
            lists.append((uk, ptr, ecol, ev, rows))
        assert any(p[i] == p[i + 1] for _, p, *_ in lists[:1] for i in range(9)) and (R == 1 or len(lists[1][0]) == 0)
        runs, keep = upload([x[:4] for x in lists])
        fk, got = dev(case["first"] + np.arange(12, dtype=np.int64)), torch.empty((12, cols), dtype=torch.int32, device="cuda")
        s.handlePushCompactRowsBatchDevice(s.format, runs, stream=st.cuda_stream)
        s.handleFetchPlanesDevice(s.format, DeviceKeys(fk.data_ptr(), 12), got.data_ptr(), None, stream=st.cuda_stream)
        assert not feed(o, kt, lists)
        st.synchronize()
        assert got.cpu().numpy().tobytes() == o.data.tobytes()
        s.flush()
        assert state(s) == ostate(o) and keep
        if both:
            singles = [push(s2, *x[:4]) for x in lists if len(x[0])]
            assert state(s2) == state(s) and singles
    finally:
        s.close()
        s2 and s2.close()


ONE = [(5, [(1, 1)])]
# (id, counters preset as (row, col, value), the runs as raw() takes them, a single call queued in front or None,
# the malformed run's expected key or None); every other counter starts at 5. Rows are shard rows of a 40-row
# store of W = 1030 columns: row 40 is last + 1 and row -1 is first - 1.
VERDICTS = [
    ("run0-negative-run1-restores", [], [[(3, [(4, -6)]), (8, [(0, 1)])], [(3, [(4, 7)])]], None, None),
    ("second-slice-of-middle-key-of-run1", [], [[(3, [(0, 1)]), (7, [(2, 1)])], [(3, [(0, 1)]), (7, [(2, 1), (1026, -6), (1029, 1)]), (9, [(1, 1)])],
                                                [(2, [(0, 1)]), (7, [(5, 1), (1027, 9)]), (9, [(1, 1)])]], None, None),
    ("key-below-first-in-run1", [], [ONE, [(-1, [(0, 1)]), (5, [(1, 1)])], [(6, [(0, 1)])]], None, None),
    ("key-above-last-in-run1", [], [ONE, [(5, [(1, 1)]), (39, [(1029, 1)]), (40, [(0, 1)])], [(5, [(1, 1)]), (6, [(0, 1)])]], None, None),
    ("negative-and-above-last-in-run1", [], [ONE, [(5, [(1, -7)]), (6, [(0, 1)]), (40, [(0, 1)])], [(6, [(0, 1)])]], None, None),
    ("above-last-in-run1-negative-in-run2", [], [ONE, [(5, [(1, 1)]), (40, [(0, 1)])], [(5, [(1, -20)])]], None, None),
    ("empty-range-over-negative-in-run1", [(6, 9, -3)], [ONE, [(5, [(0, 1)]), (6, []), (8, [(1, 1)])], [(8, [(1, 1)])]], None, None),
    ("keys-not-ascending-in-run1", [], [ONE, [(3, [(0, 1)]), (9, [(0, 1)]), (9, [(0, 1)]), (12, [(0, 1)])], [(6, [(0, 1)])]], None, 9),
    ("ptr-decreasing-in-run1", [], [ONE, [(3, [(0, 1), (1, 1)]), (9, [(0, 1)]), (12, [(0, 1)])], [(6, [(0, 1)])]], None, -1),
    ("behind-a-closed-verdict", [], [ONE, [(6, [(0, 1)])]], [(5, [(1, -6)]), (7, [(0, 1)])], None),
]


@pytest.mark.parametrize("name,preset,lsts,front,bad", VERDICTS, ids=[v[0] for v in VERDICTS])
def test_verdicts(co, oracle, name, preset, lsts, front, bad):
    """The batch on a side stream and the flush: values, the error triple and the closed store against the oracle.
    A malformed run is one the oracle is never fed: it closes with (DML_E_INVALID_ARG, key or -1, -1)."""
    case, st = fc._case("i32", 1, 1, 0, W, 40, BIG33), torch.cuda.Stream()
    init = np.full((40, W), 5, np.int32)
    for r, c_, x in preset:
        init[r, c_] = x
    s, o = pair(case, oracle, np.full((40, W), 5, np.int32))
    try:
        s.readAll(init.astype(">i4").tobytes())  # unchecked, like the reference's readAll
        assert o.read_all(init.astype(">i4").tobytes()) == 0
        lists = [raw(case["first"], lst) for lst in lsts]
        if name.startswith("ptr-"):
            lists[1][1][[1, 2]] = lists[1][1][[2, 1]]
        runs, keep = upload([x[:4] for x in lists])
        pre = [raw(case["first"], front)] if front else []
        assert feed(o, 1, pre + (lists[:1] if bad is not None else lists)) == (bad is None)
        with pytest.raises(Exception):
            if front:  # behind a long fill on the caller's stream, so that the batch is queued before the single call's verdict lands
                one, k1 = upload([pre[0][:4]])
                with torch.cuda.stream(st):
                    keep += k1 + [torch.empty(1 << 29, dtype=torch.int32, device="cuda").fill_(1)]
                s.handlePushCompactRowsDevice(s.format, *one[0], stream=st.cuda_stream)
            s.handlePushCompactRowsBatchDevice(s.format, runs, stream=st.cuda_stream)
            s.flush()
        want = o.error() if bad is None else (_lib.DML_E_INVALID_ARG, case["first"] + bad if bad >= 0 else -1, -1)
        assert s.error_state() == want and s.values().tobytes() == o.data.tobytes() and keep
        with pytest.raises(Exception):  # closed until clear_error
            s.handlePushCompactRowsBatchDevice(s.format, runs)
        s.clear_error(), o.clear_error()
        good = raw(case["first"], [(0, [(0, 1)]), (20, [(W - 1, 1)])])  # rows no case touches
        runs, keep = upload([good[:4]])
        s.handlePushCompactRowsBatchDevice(s.format, runs)
        assert not feed(o, 1, [good]) and state(s) == ostate(o) and keep
    finally:
        s.close()


def test_non_canonical_and_long(co, oracle):
    """Run 1 lists key 4 with 3 000 entries, columns repeated, unordered and one outside the row; runs 0 and 2 list it too."""
    case, rng = fc._case("i32", 1, 1, 0, W, 40, BIG33), np.random.default_rng(4)
    s, o = pair(case, oracle, np.full((40, W), 2 ** 20, np.int32))
    try:
        big = list(zip(rng.integers(0, W, 3000).tolist(), rng.integers(-99, 99, 3000).tolist()))
        big[1500] = (W, 7)
        lists = [raw(case["first"], lst) for lst in ([(4, [(7, 2), (3, 1), (7, 3), (-1, 9)]), (9, [(1, 1)])],
                                                     [(2, [(1029, 1)]), (4, big), (5, [])], [(4, [(1029, -1), (0, 1)])])]
        runs, keep = upload([x[:4] for x in lists])
        s.handlePushCompactRowsBatchDevice(s.format, runs)
        assert not feed(o, 1, lists) and state(s) == ostate(o) and keep
    finally:
        s.close()


def test_refusals(co, oracle):
    """Every refusal of the header with no state changed, the two empty forms, then a good call."""
    L, X = _lib.load(), _lib.DML_COMPACT_ROWS_BATCH_MAX_RUNS
    mat = fc._case("i32", 1, 1, 0, W, 40, BIG33)
    others = [fc._case("f32", 1, 0, 1, 5, 40, 1000), fc._case("ai32", 0, 0, 0, 1, 40, geom.NEG32)]
    s, o = pair(mat, oracle, np.full((40, W), 5, np.int32))
    rest = [make_store(others[0], fc.build_init(others[0], plain=True)), make_store(others[1], np.full((40, 1), 5, np.int32))]
    try:
        lists = [raw(mat["first"], [(5, [(1, 1)]), (7, [(0, 2)])]), raw(mat["first"], [(5, [(1, 3)])])]
        runs, keep = upload([x[:4] for x in lists])
        k, p, c, v = ([r[0].ptr if i == 0 else r[i] for r in runs] for i in range(4))
        m = [2, 1]

        def call(h, n, ks=k, ps=p, cs=c, vs=v, ms=m):
            arr = [x if x is None else (C.c_void_p * len(x))(*x) for x in (ks, ps, cs, vs)]
            return L.dml_store_push_compact_rows_batch_device(h, n, *arr, ms if ms is None else (C.c_int64 * len(ms))(*ms), None)

        before = [x.values().tobytes() for x in [s] + rest]
        bad = [(None, 2), (s._h, -1), (s._h, X + 1, k * 33, p * 33, c * 33, v * 33, m * 33), (s._h, 2, None), (s._h, 2, k, None),
               (s._h, 2, k, p, None), (s._h, 2, k, p, c, None), (s._h, 2, k, p, c, v, None), (s._h, 2, k, p, c, v, [2, -1]),
               (s._h, 2, k, p, c, v, [2, 1 << 31]), (s._h, 2, [k[0], None]), (s._h, 2, k, p, [None, c[1]]), (s._h, 2, [k[0] + 4, k[1]]),
               (s._h, 2, k, [p[0], p[1] + 2]), (s._h, 2, k, p, c, [v[0] + 2, v[1]]), (s._h, 2, k, p, c, v, [1 << 30, 1 << 30])]
        for args in bad:
            assert call(*args) == _lib.DML_E_INVALID_ARG, args[1:]
        for x in rest:
            assert call(x._h, 2) == _lib.DML_E_UNSUPPORTED
        assert call(s._h, 0, None, None, None, None, None) == 0 and call(s._h, 2, [None] * 2, [None] * 2, [None] * 2, [None] * 2, [0, 0]) == 0
        assert [x.values().tobytes() for x in [s] + rest] == before and all(x.error_state()[0] == 0 for x in [s] + rest)
        assert call(s._h, 2) == 0 and not feed(o, 1, lists) and state(s) == ostate(o) and keep
    finally:
        [x.close() for x in [s] + rest]

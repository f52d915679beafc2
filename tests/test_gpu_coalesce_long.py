"""The coalescer's long-segment path (k_co_long_list, k_co_sum_long, k_co_sum_long_narrow;
Coalescer.set_long_min / route) against the numpy model, byte for byte, with the arenas,
guard bands and input checks of tests/test_gpu_coalesce.py's `check`. The threshold is lowered
to T = 2 x DML_COALESCE_LONG_TILE so that the segments stay short; the default has its own test.
"""
import ctypes as C

import numpy as np
import pytest

import coalesce_expect as ce
import geom
from test_gpu_coalesce import _gpu, check, desc  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NEVER = 1 << 31


def sizes():
    from distml_amd import _lib
    return 2 * _lib.DML_COALESCE_LONG_TILE, _lib.DML_COALESCE_LONG_TILE


@pytest.fixture(scope="module")
def lo():
    """A context of its own with the threshold at T."""
    from distml_amd import Coalescer
    c = Coalescer(0)
    c.set_long_min(sizes()[0])
    yield c
    c.close()


def seg_keys(first, lens, seed=0):
    """A shuffled list in which key first + 3 i occurs lens[i] times, beside a key that occurs once."""
    ks = []
    for i, ln in enumerate(lens):
        ks += [first + 3 * i] * ln + [first + 3 * i + 1]
    return np.array(ks, np.int64)[np.random.default_rng(seed).permutation(len(ks))]


def edge_keys(first, narrow, seed=0):
    T, tile = sizes()
    return seg_keys(first, [T - 1, T, T + 1, T + tile - 1, T + tile, 3 * tile + 1] +
                    ([T + 63, T + 64, T + 65] if narrow else []), seed)


def routed(keys, T):
    n = np.unique(keys, return_counts=True)[1]
    return int((n >= T).sum()), int(n[n >= T].sum())


# (id, data type, key type, value type, cols, AdaGrad, first key)
LAYOUTS = [("f32-c200", 1, 1, 1, 200, False, geom.BIG33), ("f32-c50", 1, 0, 1, 50, False, geom.NEG32),
           ("f32-c257", 1, 1, 1, 257, False, geom.BIG33), ("f32-c1030", 1, 0, 1, 1030, False, geom.NEG32),
           ("f64-c129", 1, 0, 3, 129, False, 1000), ("i32-c1000", 1, 1, 0, 1000, False, geom.BIG33),
           ("ada-c200", 1, 1, 1, 200, True, geom.BIG33), ("af32", 0, 1, 1, 1, False, geom.BIG33),
           ("f32-c3", 1, 0, 1, 3, False, geom.NEG32), ("af64", 0, 0, 3, 1, False, geom.NEG32),
           ("ai32", 0, 1, 0, 1, False, geom.BIG33)]


@pytest.mark.parametrize("i", range(len(LAYOUTS)), ids=[l[0] for l in LAYOUTS])
def test_edges(lo, i):
    """Segments of T - 1 (the walk's), T, T + 1, T + TILE - 1, T + TILE and 3 x TILE + 1 occurrences
    (narrow rows: also T + 63, + 64, + 65) in one shuffled list: whole, ragged and 4-byte last
    slices, rows of several slices, the three value types; leads rotate, inputs against outputs."""
    tag, dt, kt, vt, cols, ada, first = LAYOUTS[i]
    rowcols = cols if dt == 1 else 1
    keys = edge_keys(first, rowcols * ce.VDT[vt]().itemsize < 16, seed=i)
    v = ce.values(vt, len(keys), rowcols, seed=i)
    check(lo, desc(dt, kt, vt, ada), cols, keys, v, geom.LEADS[i % 4], geom.LEADS[(i + 1 + i // 4) % 4], what=(tag,))
    assert lo.route() == routed(keys, sizes()[0]), tag


def special_long(vt):
    """Two keys of T + TILE + 1 occurrences, interleaved, 4 columns. Key 5: +Inf as the last row
    of the first tile and -Inf as the first of the next; one NaN payload; a signalling NaN;
    -0.0 only. Key 9: 2^24 (2^53), 1, 1 and 1, 1, 2^24 across the tile boundary, zeros around
    them. int32: INT_MAX + 1 across it."""
    T, tile = sizes()
    L = T + tile + 1
    keys = np.tile(np.array([5, 9], np.int64), L)
    A, B = np.arange(L) * 2, np.arange(L) * 2 + 1
    v = ce.values(vt, 2 * L, 4, seed=vt)
    if vt == 0:
        v[A, 0] = 0
        v[A[tile - 1], 0], v[A[tile], 0] = 0x7FFFFFFF, 1
        return keys, v
    u = np.uint32 if vt == 1 else np.uint64
    big = 2.0 ** 24 if vt == 1 else 2.0 ** 53
    v[A, 0], v[A, 3], v[B, 0], v[B, 1] = 0.0, -0.0, 0.0, 0.0
    v[A[tile - 1], 0], v[A[tile], 0] = np.inf, -np.inf
    v.view(u)[A[tile + 5], 1] = 0x7FC12345 if vt == 1 else 0x7FF8123456789ABC
    v.view(u)[A[3], 2] = 0x7FA00001 if vt == 1 else 0x7FF4000000000001
    v[B[tile - 2:tile + 1], 0] = [big, 1.0, 1.0]
    v[B[tile - 2:tile + 1], 1] = [1.0, 1.0, big]
    return keys, v


@pytest.mark.parametrize("vt", [1, 3, 0], ids=["f32", "f64", "i32"])
def test_special_values(lo, vt):
    """The value edge cases inside a long segment, in k_co_sum_long (4 columns) and, column by
    column, in the one-wave-per-key kernel: the model's bytes, which hold the reference's
    negative quiet NaN, +0.0 for the -0.0 column and the order's last bit."""
    keys, v = special_long(vt)
    sums = ce.coalesce(keys, v)[2]
    if vt == 0:
        assert sums[0, 0] == -(1 << 31)
    else:
        bits = sums.view(np.uint32 if vt == 1 else np.uint64)
        assert bits[0, 0] == (0xFFC00000 if vt == 1 else 0xFFF8000000000000) and bits[0, 3] == 0
        assert sums[1, 1] - sums[1, 0] == 2.0
    check(lo, desc(1, 1, vt), 4, keys, v, 4, 12, what=("specials",))
    assert lo.route() == (2, len(keys))
    for c in range(4):
        check(lo, desc(0, 0, vt), 1, keys, np.ascontiguousarray(v[:, c:c + 1]), 12, 4, what=("specials", c))
        assert lo.route() == (2, len(keys))


@pytest.mark.parametrize("dt,cols", [(1, 200), (0, 1)], ids=["f32-c200", "af32"])
def test_both_paths(dt, cols):
    """One input with the threshold at T and at never: equal bytes, route (k, occurrences) then
    (0, 0); then at T on a non-default stream, twice: equal bytes again."""
    from distml_amd import Coalescer
    T, _ = sizes()
    keys = edge_keys(geom.BIG33, cols == 1, seed=7)
    v = ce.values(1, len(keys), cols, seed=7)
    co = Coalescer(0)
    try:
        co.set_long_min(T)
        long = check(co, desc(dt, 1, 1), cols, keys, v, 4, 8, what=("long",))
        assert co.route() == routed(keys, T) and co.route()[0] >= 5
        co.set_long_min(NEVER)
        assert check(co, desc(dt, 1, 1), cols, keys, v, 4, 8, what=("walk",)) == long
        assert co.route() == (0, 0)
        co.set_long_min(T)
        st = torch.cuda.Stream()
        for rep in range(2):
            assert check(co, desc(dt, 1, 1), cols, keys, v, 4, 8, stream=st.cuda_stream, what=("stream", rep)) == long
            assert co.route() == routed(keys, T)
    finally:
        co.close()


def test_default_threshold():
    """No setter call: of segments of DML_COALESCE_LONG_MIN and DML_COALESCE_LONG_MIN - 1
    occurrences the first alone takes the long path."""
    from distml_amd import Coalescer, _lib
    D = _lib.DML_COALESCE_LONG_MIN
    keys = seg_keys(geom.NEG32, [D, D - 1], seed=2)
    co = Coalescer(0)
    try:
        check(co, desc(1, 0, 1), 4, keys, ce.values(1, len(keys), 4, seed=2), 8, 4, what=("default",))
        assert co.route() == (1, D)
    finally:
        co.close()


def test_refusals():
    """Null context, negative threshold, null out, route before a completed call; 0 and 2^40 pass."""
    from distml_amd import Coalescer, _lib
    L, E = _lib.load(), _lib.DML_E_INVALID_ARG
    out = (C.c_int64 * 2)(-7, -7)
    co = Coalescer(0)
    try:
        assert L.dml_coalescer_set_long_min(None, 5) == E and L.dml_coalescer_set_long_min(co._h, -1) == E
        assert L.dml_coalescer_set_long_min(co._h, 0) == 0 and L.dml_coalescer_set_long_min(co._h, 1 << 40) == 0
        assert L.dml_diag_coalesce_route(None, out) == E and L.dml_diag_coalesce_route(co._h, None) == E
        assert L.dml_diag_coalesce_route(co._h, out) == E and tuple(out) == (-7, -7)
    finally:
        co.close()

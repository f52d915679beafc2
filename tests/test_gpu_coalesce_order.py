"""The coalescer's bounded order stage (Coalescer.set_key_range; dml_coalesce_order.hip), byte
for byte and with no tolerance: at small n against the numpy model (tests/coalesce_expect.py),
at large n against the same call on a context with no range declared, the library sort's path.
Outputs lie in geom.OutArena poison and every byte outside the contract's stays poison."""
import numpy as np
import pytest

import coalesce_expect as ce
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def cos():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from distml_amd import Coalescer
    pair = Coalescer(0), Coalescer(0)
    yield pair
    for c in pair:
        c.close()


def desc(dt, kt, vt):
    from distml_amd import DataDesc
    return DataDesc(dt, kt, vt, False, True, False)


def lib():
    from distml_amd import _lib
    return _lib


def passes(span):
    bits = max(1, int(span - 1).bit_length())
    p = -(-bits // lib().DML_COALESCE_ORDER_BITS)
    return (1, p, 0) if p <= lib().DML_COALESCE_ORDER_MAX_PASSES else (0, 0, 0)


def run(co, fmt, cols, keys, v, model=True):
    """One Coalescer.run into poisoned arenas sized for n rows: the guard bands are checked and
    (model) the outputs compared with the numpy model. Returns (keys, sums, inverse) bytes."""
    from distml_amd import DeviceKeys
    n, rowb = len(keys), v.shape[1] * v.itemsize
    ka, va = geom.pack([keys.tobytes()], 8), geom.pack([v.tobytes()], 4)
    outs = [geom.OutArena(n * 8, 8).upload(), geom.OutArena(n * rowb, 12).upload(), geom.OutArena(n * 4, 4).upload()]
    m = co.run(fmt, cols, DeviceKeys(ka.ptrs[0], n), va.ptrs[0], outs[0].ptr, outs[1].ptr, outs[2].ptr, n)
    got = []
    for a, nb in zip(outs, (m * 8, m * rowb, n * 4)):
        got.append(a.read()[:nb].tobytes())
        a.untouched([(0, nb)])
    ka.check(), va.check()
    if model:
        uk, inv, sums = ce.coalesce(keys, v)
        assert got == [uk.tobytes(), sums.tobytes(), inv.tobytes()]
    return got


SPANS = [200, (1 << 8) + 1, (1 << 16) + 1, (1 << 24) + 1, 1 << 32]


@pytest.mark.parametrize("span", SPANS, ids=lambda s: "span%d" % s)
@pytest.mark.parametrize("lay", [(1, 0, 1, 3), (1, 1, 1, 200), (1, 1, 3, 5)], ids=["f32-c3", "f32-c200", "f64-c5-i64"])
def test_passes_and_key_placement(cos, lay, span):
    """1 to 4 passes, first keys below zero and past 2^33, the range's first and last key both
    listed, and the patterns where stability decides float bits."""
    dt, kt, vt, cols = lay
    n = 300
    for first in (geom.NEG32, geom.BIG33):
        cos[0].set_key_range(first, first + span)
        pats = ce.patterns(first, n, lib().DML_COALESCE_DEPTH, lib().DML_COALESCE_BATCH, seed=span % 97)
        for i, name in enumerate(("equal", "two", "random")):
            keys = pats[name].copy()
            keys[5::7] += (span - 1) - (keys[5::7] - first)  # a seventh of the list is the last key
            keys[3], keys[n // 2] = first, first + span - 1
            run(cos[0], desc(dt, kt, vt), cols, keys, ce.values(vt, n, cols, seed=i))
            assert cos[0].order_route() == passes(span), (name, first)


@pytest.mark.parametrize("span", [200, (1 << 16) + 1], ids=["p1", "p3"])
@pytest.mark.parametrize("edge", [-1, 0, 1, "2t+5"])
def test_tile_edges(cos, edge, span):
    """n around one tile and past two; all-equal keys and the range's two end keys alternating,
    so that ranks cross rounds, waves and tiles in every pass."""
    T = lib().DML_COALESCE_ORDER_TILE
    n = 2 * T + 5 if edge == "2t+5" else T + edge
    first = geom.BIG33
    cos[0].set_key_range(first, first + span)
    for keys in (np.full(n, first + span - 1, np.int64), first + (np.arange(n, dtype=np.int64) & 1) * (span - 1)):
        run(cos[0], desc(0, 1, 1), 1, keys, ce.values(1, n, 1, seed=n))
        assert cos[0].order_route() == passes(span)


def test_several_tiles_per_block(cos):
    """More tiles than blocks: a block carries its bases over a run of tiles, the runs uneven; random keys over a
    3-pass span with a few hot keys. Yardstick: the undeclared call. The declared call again gives equal bytes."""
    T, B = lib().DML_COALESCE_ORDER_TILE, lib().DML_COALESCE_ORDER_MAX_BLOCKS
    n, span, first = 2 * B * T + T + 5, (1 << 16) + 1, geom.NEG32
    rng = np.random.default_rng(15)
    keys = first + rng.integers(0, span, size=n).astype(np.int64)
    keys[rng.integers(0, n, size=n // 8)] = first + 77
    keys[rng.integers(0, n, size=n // 16)] = first + span - 1
    v = ce.values(1, n, 1, seed=2)
    cos[0].set_key_range(first, first + span)
    got = run(cos[0], desc(0, 1, 1), 1, keys, v, model=False)
    assert cos[0].order_route() == passes(span)
    assert got == run(cos[1], desc(0, 1, 1), 1, keys, v, model=False) and cos[1].order_route() == (0, 0, 0)
    assert got == run(cos[0], desc(0, 1, 1), 1, keys, v, model=False)


@pytest.mark.parametrize("bad", ["last", "first-1", "min", "max"])
def test_the_hint_is_only_a_hint(cos, bad):
    """A key outside the declared range: the outputs are the model's, the route says the order
    was redone, and on a DML_E_CAPACITY call every output byte stays poison."""
    T = lib().DML_COALESCE_ORDER_TILE
    n, span, first = T + 300, (1 << 8) + 1, geom.BIG33
    keys = first + np.random.default_rng(3).integers(0, span, size=n).astype(np.int64)
    keys[n - 2] = {"last": first + span, "first-1": first - 1, "min": ce.INT64_MIN, "max": ce.INT64_MAX}[bad]
    v = ce.values(1, n, 3, seed=4)
    cos[0].set_key_range(first, first + span)
    run(cos[0], desc(1, 1, 1), 3, keys, v)
    assert cos[0].order_route() == (0, 0, 1)
    m = len(np.unique(keys))
    ka, va = geom.pack([keys.tobytes()], 0), geom.pack([v.tobytes()], 4)
    outs = [geom.OutArena(n * 8, 8).upload(), geom.OutArena(n * 12, 12).upload(), geom.OutArena(n * 4, 4).upload()]
    assert ce.raw_call(lib().load(), cos[0]._h.value, desc(1, 1, 1), 3, ka.ptrs[0], n, va.ptrs[0], outs[0].ptr, outs[1].ptr,
                       outs[2].ptr, m - 1) == (lib().DML_E_CAPACITY, m)
    for a in outs:
        a.read(), a.untouched([])


def test_the_three_calls(cos):
    """Keys-only run, run_packed and run_elems with a range declared write the bytes of the same
    calls undeclared."""
    from distml_amd import DeviceKeys, record_bytes
    n, span, first, cols = 5000, (1 << 8) + 1, geom.NEG32, 40
    rng = np.random.default_rng(9)
    keys = torch.from_numpy(first + rng.integers(0, span, size=n).astype(np.int64)).cuda()
    v = torch.from_numpy(ce.values(1, n, cols, seed=1)).cuda()
    ec = torch.from_numpy(rng.integers(0, cols, size=(n, 2)).astype(np.int32)).cuda()
    ev = torch.from_numpy(rng.integers(-3, 4, size=(n, 2)).astype(np.int32)).cuda()
    ffmt, ifmt = desc(1, 0, 1), desc(1, 0, 0)
    R = record_bytes(ffmt, cols)[0]
    cos[0].set_key_range(first, first + span)
    got = []
    for co in cos:
        ko, io = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        rec, erec = (torch.zeros(n * R // 4, dtype=torch.int32, device="cuda") for _ in range(2))
        dk = DeviceKeys(keys.data_ptr(), n)
        res = [co.run(ffmt, cols, dk, None, ko.data_ptr(), None, io.data_ptr(), n), co.order_route()]
        res += [co.run_packed(ffmt, cols, dk, v.data_ptr(), rec.data_ptr(), n * R), co.order_route()]
        res += [co.run_elems(ifmt, cols, dk, ec.data_ptr(), ev.data_ptr(), 2, erec.data_ptr(), n * R, records=True),
                co.order_route()]
        torch.cuda.synchronize()
        got.append((res, [t.cpu().numpy().tobytes() for t in (ko, io, rec, erec)]))
    assert got[0][0][1::2] == [passes(span)] * 3 and got[1][0][1::2] == [(0, 0, 0)] * 3
    assert got[0][0][0::2] == got[1][0][0::2] and got[0][1] == got[1][1]

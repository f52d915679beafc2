"""The device gradient coalescer (dml_coalesce_device; the wrapper Coalescer.run) against its
numpy model (tests/coalesce_expect.py, pinned to the CPU oracle by tests/test_coalesce_expect.py),
byte for byte: no tolerance anywhere.

Every output is a geom.OutArena (placed at base + GUARD + lead inside poison; the key plane,
8-byte aligned, at leads 0 and 8), sized for cap_rows rows, read back, compared, and every
byte outside the contract's m x 8, m x cols x V and n x 4 bytes must still be poison. Every
input is a geom.Arena (poison around it, its own lead) and is compared unchanged afterwards.
The coalescer has no knob: its kernel is chosen by the value type and the row width alone.
"""
import numpy as np
import pytest

import coalesce_expect as ce
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


@pytest.fixture(scope="module")
def co():
    from distml_amd import Coalescer
    c = Coalescer(0)
    yield c
    c.close()


def tiles():
    from distml_amd import _lib
    return _lib.DML_COALESCE_BLOCK_KEYS, _lib.DML_COALESCE_BATCH, _lib.DML_COALESCE_DEPTH


def desc(dt, kt, vt, ada=False):
    from distml_amd import DataDesc
    return DataDesc(dt, kt, vt, False, True, ada)


def same(got, want, what):
    want = np.frombuffer(want, np.uint8)
    assert got.size == want.size, (what, got.size, want.size)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError((what, "first differing byte", int(bad[0]), "of", want.size, "count", int(bad.size)))


def check(co, fmt, cols, keys, values, lead=0, in_lead=0, extra_cap=0, inverse=True, stream=None, what=()):
    """One run: outputs sized for m + extra_cap rows between poison, everything compared with
    the model, guard bands and inputs checked. Returns the three output byte strings."""
    from distml_amd import DeviceKeys
    n = len(keys)
    rowcols = cols if fmt.dataType == 1 else 1
    uk, inv, sums = ce.coalesce(keys, values)
    m = len(uk)
    cap = m + extra_cap
    rowb = 0 if values is None else rowcols * values.dtype.itemsize
    ka = geom.pack([keys.tobytes()], in_lead & 8)
    va = geom.pack([values.tobytes()], in_lead) if values is not None else None
    ko = geom.OutArena(cap * 8, lead & 8).upload()
    vo = geom.OutArena(cap * rowb, lead).upload() if values is not None else None
    io = geom.OutArena(n * 4, (lead + 8) % 16).upload() if inverse else None
    got_m = co.run(fmt, cols, DeviceKeys(ka.ptrs[0], n), va.ptrs[0] if va else None, ko.ptr, vo.ptr if vo else None,
                   io.ptr if io else None, cap, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    assert got_m == m, (what, got_m, m)
    out = []
    same(ko.read()[:m * 8], uk.tobytes(), ("keys",) + tuple(what))
    ko.untouched([(0, m * 8)])
    out.append(ko.back[ko.off:ko.off + m * 8].tobytes())
    if vo is not None:
        same(vo.read()[:m * rowb], sums.tobytes(), ("values",) + tuple(what))
        vo.untouched([(0, m * rowb)])
        out.append(vo.back[vo.off:vo.off + m * rowb].tobytes())
    if io is not None:
        same(io.read(), inv.tobytes(), ("inverse",) + tuple(what))
        io.untouched([(0, n * 4)])
        out.append(io.back[io.off:io.off + n * 4].tobytes())
    ka.check()
    if va is not None:
        va.check()
    return out


# (id, data type, key type, value type, cols, AdaGrad, first key, occurrences per pattern)
LAYOUTS = [("af32", 0, 1, 1, 1, False, geom.BIG33, 700), ("f32-c3", 1, 0, 1, 3, False, geom.NEG32, 700),
           ("f32-c50", 1, 0, 1, 50, False, geom.NEG32, 500), ("f32-c200", 1, 1, 1, 200, False, geom.BIG33, 300),
           ("f32-c256", 1, 0, 1, 256, False, 1000, 300), ("f32-c257", 1, 1, 1, 257, False, geom.BIG33, 300),
           ("f32-c1024", 1, 0, 1, 1024, False, geom.NEG32, 150), ("f32-c1030", 1, 1, 1, 1030, False, geom.BIG33, 150),
           ("af64", 0, 0, 3, 1, False, geom.NEG32, 700), ("f64-c5", 1, 1, 3, 5, False, geom.BIG33, 500),
           ("f64-c129", 1, 0, 3, 129, False, 1000, 300),
           ("ai32", 0, 1, 0, 1, False, geom.BIG33, 700), ("i32-c7", 1, 0, 0, 7, False, geom.NEG32, 500),
           ("i32-c1000", 1, 1, 0, 1000, False, geom.BIG33, 150),
           ("ada-c200", 1, 1, 1, 200, True, geom.BIG33, 300)]


@pytest.mark.parametrize("lay", LAYOUTS, ids=lambda l: l[0])
def test_layouts(co, lay):
    """Every row width class (one lane per key; groups of 1 to 64 lanes, whole and ragged rows;
    rows of two to five 1-KiB spans whose last span is whole, 4 bytes or 24 bytes), the three value
    types, an AdaGrad desc, int32- and int64-key descs with first keys below zero and past
    2^33. Key patterns: all distinct ascending (m = n, inverse = identity), all distinct
    permuted (with INT64_MIN and INT64_MAX as keys), all equal (m = 1), two keys alternating,
    random repeats, and the skewed list whose longest segments have DML_COALESCE_DEPTH -+ 1,
    DML_COALESCE_BATCH - 1 / + 0 / + 1 and 2 x BATCH + 1 occurrences next to segments of 1.
    Leads rotate over the patterns, inputs against outputs."""
    tag, dt, kt, vt, cols, ada, first, n = lay
    _, batch, depth = tiles()
    fmt = desc(dt, kt, vt, ada)
    pats = ce.patterns(first, n, depth, batch, seed=len(tag))
    pats["perm"][3], pats["perm"][n // 2] = ce.INT64_MAX, ce.INT64_MIN
    assert sorted(np.unique(pats["skewed"], return_counts=True)[1].tolist())[-6:] == \
        [depth - 1, depth + 1, batch - 1, batch, batch + 1, 2 * batch + 1]
    for i, (name, keys) in enumerate(pats.items()):
        v = ce.values(vt, len(keys), cols if dt == 1 else 1, seed=i)
        lead, in_lead = geom.LEADS[i % 4], geom.LEADS[(i + 1 + i // 4) % 4]
        check(co, fmt, cols, keys, v, lead, in_lead, what=(tag, name))
        if name == "asc":
            assert (ce.coalesce(keys)[1] == np.arange(n)).all()


def test_heads_edges(co):
    """k_co_heads' tiling: n in {1, 63, 64, 65, BLOCK_KEYS - 1, BLOCK_KEYS, BLOCK_KEYS + 1,
    3 x BLOCK_KEYS + 5} with random repeats and all distinct; one key whose sorted run straddles a
    block boundary, one whose run starts exactly at it; all-equal keys over three blocks."""
    bk, _, _ = tiles()
    fmt = desc(1, 1, 1)
    rng = np.random.default_rng(77)
    for i, n in enumerate((1, 63, 64, 65, bk - 1, bk, bk + 1, 3 * bk + 5)):
        for name, keys in (("repeats", geom.BIG33 + rng.integers(0, max(1, n // 2), size=n).astype(np.int64)),
                           ("distinct", geom.BIG33 + rng.permutation(n).astype(np.int64))):
            check(co, fmt, 3, keys, ce.values(1, n, 3, seed=n), geom.LEADS[i % 4], geom.LEADS[(i + 2) % 4],
                  what=("edge", n, name))
    for name, keys in (("straddle", ce.heads_straddle(bk)), ("at boundary", ce.heads_at_boundary(bk)),
                       ("equal over three blocks", np.full(2 * bk + 9, -3, np.int64))):
        check(co, fmt, 3, keys, ce.values(1, len(keys), 3, seed=5), 4, 12, what=(name,))
        check(co, fmt, 3, keys, None, 8, 0, what=(name, "keys only"))


@pytest.mark.parametrize("vt,cols", [(1, 4), (3, 4), (0, 4), (1, 1), (3, 1)], ids=["f32", "f64", "i32", "af32", "af64"])
def test_special_values(co, vt, cols):
    """-0.0 alone (out: +0.0) and with a partner, NaN payloads and a signalling NaN (out:
    quiet), +Inf then -Inf, denormals, the ties-to-even triples 2^24, 1, 1 against 1, 1, 2^24
    where the order decides the last bit, int32 INT_MAX + 1; in the group kernel (4 columns)
    and, column by column, in the one-lane-per-key kernel (arrays)."""
    keys, v = ce.special_case(vt)
    if cols == 4:
        check(co, desc(1, 1, vt), 4, keys, v, 4, 12, what=("specials",))
        return
    for c in range(4):
        check(co, desc(0, 0, vt), 1, keys, np.ascontiguousarray(v[:, c:c + 1]), 12, 4, what=("specials", c))


def test_guard_bands(co):
    """Inputs and outputs at 4 and 12 mod 16 between canary words, on a ragged row (50 f32
    columns: 200 bytes, 8 mod 16) and a two-span one (257): exactly the contract's bytes change,
    and with cap_rows > m the rows past m stay canary. (Every other test here runs between
    canaries too; this one crosses the two odd leads.)"""
    _, batch, depth = tiles()
    for cols in (50, 257):
        keys = ce.patterns(geom.NEG32, 300, depth, batch, seed=cols)["random"]
        v = ce.values(1, len(keys), cols, seed=cols)
        for lead in (4, 12):
            for in_lead in (4, 12):
                check(co, desc(1, 0, 1), cols, keys, v, lead, in_lead, extra_cap=7, what=("guard", cols, lead, in_lead))


def test_capacity(co):
    """cap_rows = m - 1: DML_E_CAPACITY, *out_rows == m, and all three outputs still canary (the
    writing kernels start only after the host has seen the count). cap_rows = m passes."""
    from distml_amd import _lib
    L = _lib.load()
    fmt, cols, n = desc(1, 1, 1), 50, 900
    keys = geom.BIG33 + np.random.default_rng(4).integers(0, 301, size=n).astype(np.int64)
    v = ce.values(1, n, cols, seed=4)
    uk, inv, sums = ce.coalesce(keys, v)
    m = len(uk)
    ka, va = geom.pack([keys.tobytes()], 8), geom.pack([v.tobytes()], 4)
    ko, vo, io = (geom.OutArena(m * 8, 8).upload(), geom.OutArena(m * cols * 4, 12).upload(),
                  geom.OutArena(n * 4, 4).upload())
    st = torch.cuda.Stream()
    for stream in (None, st.cuda_stream):
        for cap in (m - 1, 0, -1):
            assert ce.raw_call(L, co._h.value, fmt, cols, ka.ptrs[0], n, va.ptrs[0], ko.ptr, vo.ptr, io.ptr, cap,
                            stream=stream) == (_lib.DML_E_CAPACITY, m), cap
        torch.cuda.synchronize()
        for a in (ko, vo, io):
            a.read()
            a.untouched([])
    assert ce.raw_call(L, co._h.value, fmt, cols, ka.ptrs[0], n, va.ptrs[0], ko.ptr, vo.ptr, io.ptr, m) == (0, m)
    same(ko.read(), uk.tobytes(), "keys")
    same(vo.read(), sums.tobytes(), "values")
    same(io.read(), inv.tobytes(), "inverse")
    ka.check()
    va.check()


def test_refusals_with_a_context(co):
    """The refusal table of tests/test_coalesce_expect.py with a real context and live arenas,
    in the synchronous and the stream form: the status, *out_rows untouched, and every arena
    still as uploaded; then the same arguments, in order, work."""
    from distml_amd import _lib
    L = _lib.load()
    n, cols = 9, 5
    keys = geom.BIG33 + np.arange(n, dtype=np.int64)
    v = ce.values(1, n, cols)
    ka, va = geom.pack([keys.tobytes()], 0), geom.pack([v.tobytes()], 4)
    ko, vo, io = geom.OutArena(n * 8, 8).upload(), geom.OutArena(n * cols * 4, 12).upload(), geom.OutArena(n * 4, 4).upload()
    K, V, KO, VO, IO = ka.ptrs[0], va.ptrs[0], ko.ptr, vo.ptr, io.ptr
    st = torch.cuda.Stream()
    for stream in (None, st.cuda_stream):
        for what, args, want in ce.refusal_cases(K, V, KO, VO, IO, n, cols):
            assert ce.raw_call(L, co._h.value, *args, stream=stream) == (want, -7), what
        assert ce.raw_call(L, co._h.value, desc(1, 1, 1), cols, K, 0, V, KO, VO, IO, n, stream=stream) == (0, 0)
    torch.cuda.synchronize()
    for a in (ko, vo, io):
        a.read()
        a.untouched([])
    ka.check()
    va.check()
    assert ce.raw_call(L, co._h.value, desc(1, 1, 1), cols, K, n, V, KO, VO, IO, n) == (0, n)
    same(vo.read(), v.tobytes(), "distinct ascending keys: the values as given")


def test_modes(co):
    """Keys-only (the KeyList half); values without the inverse; two calls on one context back
    to back on a stream with no host wait of the caller's between them, the second with a list
    several times longer (the workspace grows, and the call first waits for the one in flight),
    then a short one again; two runs of one input give equal bytes."""
    from distml_amd import Coalescer, DeviceKeys
    fmt, cols = desc(1, 0, 1), 50
    rng = np.random.default_rng(8)
    keys = geom.NEG32 + rng.integers(0, 200, size=600).astype(np.int64)
    v = ce.values(1, 600, cols, seed=8)
    check(co, fmt, cols, keys, None, 8, 8, what=("keys only",))
    check(co, fmt, cols, keys, None, 0, 0, inverse=False, what=("keys only, no inverse",))
    first = check(co, fmt, cols, keys, v, 4, 12, inverse=False, what=("no inverse",))
    assert check(co, fmt, cols, keys, v, 4, 12, inverse=False, what=("again",)) == first

    own = Coalescer(0)  # a fresh context: its workspace starts empty
    try:
        st = torch.cuda.Stream()
        runs = []
        for n in (300, 4096, 17):
            k = geom.NEG32 + rng.integers(0, max(2, n // 3), size=n).astype(np.int64)
            x = ce.values(1, n, cols, seed=n)
            uk, inv, sums = ce.coalesce(k, x)
            dk, dv = torch.from_numpy(k).cuda(), torch.from_numpy(x).cuda()
            ko, vo, io = (geom.OutArena(len(uk) * 8, 0).upload(), geom.OutArena(sums.nbytes, 4).upload(),
                          geom.OutArena(n * 4, 12).upload())
            runs.append((uk, inv, sums, dk, dv, ko, vo, io))
        torch.cuda.synchronize()
        for uk, inv, sums, dk, dv, ko, vo, io in runs:
            assert own.run(fmt, cols, DeviceKeys(dk.data_ptr(), len(inv)), dv.data_ptr(), ko.ptr, vo.ptr, io.ptr,
                           len(uk), stream=st.cuda_stream) == len(uk)
        st.synchronize()
        for uk, inv, sums, dk, dv, ko, vo, io in runs:
            same(ko.read(), uk.tobytes(), ("keys", len(inv)))
            same(vo.read(), sums.tobytes(), ("values", len(inv)))
            same(io.read(), inv.tobytes(), ("inverse", len(inv)))
            for a, nb in ((ko, uk.nbytes), (vo, sums.nbytes), (io, inv.nbytes)):
                a.untouched([(0, nb)])
        assert all(t >= 0 for t in own.stage_times())
    finally:
        own.close()


def test_stream_form(co):
    """The keys and the values are produced by torch kernels on the same non-default stream
    with no synchronise before the call; the result equals the model on what they produced."""
    from distml_amd import DeviceKeys
    n, cols = 4001, 50
    fmt = desc(1, 0, 1)
    rng = np.random.default_rng(12)
    a = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32)).cuda()
    tok = torch.from_numpy(rng.integers(0, 1 << 40, size=n).astype(np.int64)).cuda()
    ko, vo, io = geom.OutArena(n * 8, 8).upload(), geom.OutArena(n * cols * 4, 12).upload(), geom.OutArena(n * 4, 4).upload()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _ in range(20):  # enough work ahead of the call that it would run early if it did not queue
            b = b * 1.0001 + a
        grad = (a * 0.5 - b).contiguous()
        keys = (tok % 1009 - 500).contiguous()
        m = co.run(fmt, cols, DeviceKeys(keys.data_ptr(), n), grad.data_ptr(), ko.ptr, vo.ptr, io.ptr, n,
                   stream=st.cuda_stream)
    st.synchronize()
    uk, inv, sums = ce.coalesce(keys.cpu().numpy(), grad.cpu().numpy())
    assert m == len(uk) and 900 < m <= 1009
    same(ko.read()[:m * 8], uk.tobytes(), "stream keys")
    ko.untouched([(0, m * 8)])
    same(vo.read()[:sums.nbytes], sums.tobytes(), "stream values")
    vo.untouched([(0, sums.nbytes)])
    same(io.read(), inv.tobytes(), "stream inverse")
    io.untouched([(0, n * 4)])

"""The device record codec (dml_records_pack_device / dml_records_unpack_device; the wrappers
pack_push_device / unpack_fetch_device) against the host encoders and the numpy decode of the
CPU oracle's fetch, byte for byte: no tolerance anywhere.

Every output is a geom.OutArena (placed at base + GUARD + lead inside poison, all four leads;
the key plane, 8-byte aligned, at leads 0 and 8), read back, compared, and every byte outside
the stated range must still be poison. Every input is a geom.Arena (poison around it, its
own lead) and is compared unchanged afterwards. The cases and expectations are
tests/codec_cases.py, pinned on the CPU by tests/test_codec_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

import codec_cases as cc
import fetch_cases as fc
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()
    from distml_amd import _lib
    L = _lib.load()
    yield
    L.dml_diag_codec_knob(_lib.DML_CODEC_KNOB_WIDE_INDEX, 0)
    L.dml_diag_codec_knob(_lib.DML_CODEC_KNOB_LOADS, 0)


def fmt_of(case):
    from distml_amd import DataDesc
    return DataDesc(case["dt"], case["kt"], case["vt"], False, True, case["ada"])


def knob(which, value):
    from distml_amd import _lib
    assert _lib.load().dml_diag_codec_knob(which, value) == 0


def same(got, want, what):
    want = np.frombuffer(want, np.uint8)
    assert got.size == want.size, (what, got.size, want.size)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError((what, "first differing byte", int(bad[0]), "of", want.size, "count", int(bad.size)))


def pack_check(case, keys, values, out_lead, in_lead=0, what=()):
    """One synchronous pack. keys: int64 array (list form) or an int key_lo (range form)."""
    from distml_amd import DeviceKeys, pack_push_device
    n = len(values)
    if isinstance(keys, np.ndarray):
        want = cc.pack_expected(case, keys, values)
        ka = geom.pack([keys.tobytes()], 0)
        kd = DeviceKeys(ka.ptrs[0], n)
    else:
        want = cc.pack_expected(case, keys + np.arange(n, dtype=np.int64), values)
        ka, kd = None, int(keys)
    assert len(want) == n * cc.push_record_bytes(case)
    va = geom.pack([values.tobytes()], in_lead)
    out = geom.OutArena(len(want), out_lead).upload()
    got_len = pack_push_device(fmt_of(case), case["cols"], kd, va.ptrs[0], n, out.ptr, len(want), flags=cc.flags(case))
    assert got_len == len(want), (what, got_len)
    same(out.read(), want, ("pack", case["id"], out_lead, in_lead) + tuple(what))
    out.untouched([(0, len(want))])
    va.check()
    if ka is not None:
        ka.check()


PLANE_SETS = (("v", "a", "k"), ("v",), ("a",), ("k",))


def unpack_check(case, fetched, lead, in_lead=0, planes=("v", "a", "k"), what=()):
    """One synchronous unpack of the oracle's fetch bytes into the planes named."""
    from distml_amd import unpack_fetch_device
    keys, vals, alpha = cc.unpack_expected(case, fetched)
    n = len(keys)
    want = {"v": vals.tobytes(), "k": keys.tobytes()}
    if alpha is not None:
        want["a"] = alpha.tobytes()
    planes = [p for p in planes if p in want]
    if not planes:
        return
    ra = geom.pack([fetched], in_lead)
    outs = {p: geom.OutArena(len(want[p]), (lead & 8) if p == "k" else lead).upload() for p in planes}
    ptr = {p: (outs[p].ptr if p in outs else None) for p in "vak"}
    unpack_fetch_device(fmt_of(case), case["cols"], ra.ptrs[0], n, ptr["v"], ptr["a"], ptr["k"], flags=cc.flags(case))
    for p in planes:
        same(outs[p].read(), want[p], ("unpack", p, case["id"], lead, in_lead) + tuple(what))
        outs[p].untouched([(0, len(want[p]))])
    ra.check()


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c["id"])
def test_layouts(oracle, case):
    """Test 1. Every store of fetch_cases.CASES. Pack: the list form (shuffled keys with repeats,
    with keys beyond 2^32 and negative ones; one key; no key) and the range form from the
    case's first key, at the four output leads, values with -0.0, denormals, +-Inf and NaN
    payloads. Unpack: the oracle's fetch of a shuffled list with repeats, one key, no key and
    an inner range, at the four leads: all planes together at every lead, each plane alone
    at one lead per form."""
    _, o = fc.make_oracle(case, oracle)
    lists = cc.pack_key_lists(case)
    vals = {k: cc.pack_values(case, len(v)) for k, v in lists.items()}
    fetched = {k: o.fetch(v) for k, v in fc.key_lists(case).items() if k != "asc"}
    fetched["range"] = o.fetch(fc.ranges(case)["inner"][2][:97])
    for i, lead in enumerate(geom.LEADS):
        for name, keys in lists.items():
            pack_check(case, keys, vals[name], lead, what=("list", name))
        pack_check(case, case["first"], vals["shuffled"], lead, what=("range",))
        for f, (name, b) in enumerate(fetched.items()):
            unpack_check(case, b, lead, what=(name, "all"))
            alone = PLANE_SETS[1 + (i + f) % 3]
            unpack_check(case, b, lead, planes=alone, what=(name, "alone"))
    pack_check(case, case["first"], vals["none"], 4, what=("range", "none"))


CROSS = [c for c in cc.CASES if c["id"].startswith(("ada-c17-", "f64-c5-", "af32-c1-k8", "ai32-c1-k4"))]


@pytest.mark.parametrize("case", CROSS, ids=lambda c: c["id"])
def test_input_leads_cross_output_leads(oracle, case):
    """Test 1, the 16-combination cross: dev_values / dev_records at the four leads against the
    four output leads, on two matrix cases (AdaGrad at 17 columns, f64 at 5) and two arrays."""
    assert len(CROSS) == 4
    _, o = fc.make_oracle(case, oracle)
    keys = cc.pack_key_lists(case)["shuffled"]
    vals = cc.pack_values(case, len(keys))
    fetched = o.fetch(fc.key_lists(case)["shuffled"][:173])
    for in_lead in geom.LEADS:
        for lead in geom.LEADS:
            pack_check(case, keys, vals, lead, in_lead)
            unpack_check(case, fetched, lead, in_lead)


@pytest.mark.parametrize("case", [cc.EDGE_CASE, cc.EDGE_ARRAY], ids=lambda c: c["id"])
def test_tiling_edges(oracle, case):
    """Test 2. 24-byte records (5 f32 columns, int32 keys) and 12-byte array records (f64,
    int32 keys). Pack: the stream ends one record before, at and one record past three whole
    wave runs (DML_CODEC_WAVE_BYTES) and one whole block (DML_CODEC_BLOCK_BYTES); unpack: the
    values plane ends there. List and range form, four leads (a lead moves every line
    boundary by 4, 8 or 12 bytes against the records), and n = 1."""
    from distml_amd import _lib
    W, B = _lib.DML_CODEC_WAVE_BYTES, _lib.DML_CODEC_BLOCK_BYTES
    rec = cc.push_record_bytes(case)
    ns_pack = fc.edge_counts(W, B) if rec == 24 else cc.edge_counts(rec, W, B)
    assert ns_pack == cc.edge_counts(rec, W, B)
    ns_unpack = cc.edge_counts(case["cols"] * cc.value_bytes(case), W, B)
    _, o = fc.make_oracle(case, oracle)
    rng = np.random.default_rng(5)
    for n in ns_pack + [1]:
        keys = case["first"] + rng.permutation(case["rows"])[:n].astype(np.int64)
        vals = cc.pack_values(case, n, seed=n)
        for lead in geom.LEADS:
            pack_check(case, keys, vals, lead, what=("edge list", n))
            pack_check(case, case["first"] + 3, vals, lead, what=("edge range", n))
    for n in ns_unpack + [1]:
        fetched = o.fetch(case["first"] + rng.permutation(case["rows"])[:n].astype(np.int64))
        for lead in geom.LEADS:
            unpack_check(case, fetched, lead, what=("edge", n))


# Record lengths on each side of the load-path thresholds of dml_codec.hip. kPackVloadMinDw = 80
# dwords: f32 behind int32 keys at 78 and 79 columns (79 and 80 dwords). kUnpackPairVloadMinDw
# = 17 dwords of AdaGrad's fetch record: 7 columns behind an int64 key (16) and 8 behind an
# int32 key (17). Plain unpack has no threshold (it never takes the 16-byte loads by itself);
# the other lengths run both paths through the knob: the neighbours of k_fetch_vec's and
# k_pull_unsplit's thresholds, an f64 row, and AdaGrad at odd and even cols.
LOAD_CASES = [fc._case("f32", 1, 0, 1, c, 64, 1000) for c in (78, 79, 319, 320, 767, 768)] + \
             [fc._case("f64", 1, 1, 3, 129, 64, geom.BIG33), fc._case("ada", 1, 1, 1, 7, 64, geom.BIG33, True)] + \
             [fc._case("ada", 1, 0, 1, c, 64, 1000, True) for c in (8, 127, 128, 201, 384)]


@pytest.mark.parametrize("case", LOAD_CASES, ids=lambda c: c["id"])
def test_load_paths(oracle, case):
    """Test 3. Each record length under the shipped choice of loads (knob 0), with every dword
    gathered singly (1) and with 16-byte loads wherever a line lies inside one row (2): the
    same bytes. AdaGrad with odd and even cols (an odd count moves the pairs against the
    lines from record to record)."""
    from distml_amd import _lib
    _, o = fc.make_oracle(case, oracle)
    keys = case["first"] + np.random.default_rng(9).permutation(case["rows"])[:23].astype(np.int64)
    vals = cc.pack_values(case, len(keys))
    fetched = o.fetch(keys)
    try:
        for loads in (0, 1, 2):
            knob(_lib.DML_CODEC_KNOB_LOADS, loads)
            for lead in geom.LEADS:
                pack_check(case, keys, vals, lead, in_lead=(lead + 4) % 16, what=("loads", loads))
                unpack_check(case, fetched, lead, in_lead=(lead + 8) % 16, what=("loads", loads))
    finally:
        knob(_lib.DML_CODEC_KNOB_LOADS, 0)


def test_forced_wide_index(oracle):
    """Test 4b. The kernels divide a line's first dword by the record (row) length in 32 bits
    while the stream (plane) is under 2^32 dwords; DML_CODEC_KNOB_WIDE_INDEX = 1 runs the
    64-bit division a longer one takes, on small cases, with both load paths."""
    from distml_amd import _lib
    try:
        knob(_lib.DML_CODEC_KNOB_WIDE_INDEX, 1)
        for case in (cc.EDGE_CASE, cc.EDGE_ARRAY, fc._case("ada", 1, 1, 1, 50, 301, geom.BIG33, True),
                     fc._case("af32ref", 0, 0, 1, 1, 1237, 1000, False, True)):
            _, o = fc.make_oracle(case, oracle)
            keys = fc.key_lists(case)["shuffled"][:211]
            vals = cc.pack_values(case, len(keys))
            fetched = o.fetch(keys)
            for loads in (1, 2):
                knob(_lib.DML_CODEC_KNOB_LOADS, loads)
                for lead in geom.LEADS:
                    pack_check(case, keys, vals, lead, what=("wide", loads))
                    unpack_check(case, fetched, lead, what=("wide", loads))
    finally:
        knob(_lib.DML_CODEC_KNOB_WIDE_INDEX, 0)
        knob(_lib.DML_CODEC_KNOB_LOADS, 0)
    assert _lib.load().dml_diag_codec_knob(_lib.DML_CODEC_KNOB_WIDE_INDEX, 2) == _lib.DML_E_INVALID_ARG
    assert _lib.load().dml_diag_codec_knob(_lib.DML_CODEC_KNOB_LOADS, 3) == _lib.DML_E_INVALID_ARG
    assert _lib.load().dml_diag_codec_knob(7, 0) == _lib.DML_E_INVALID_ARG


def test_stream_past_4_gib():
    """Test 4a. 1 048 700 records of 1 025 dwords (int32 key, 1 024 f32 columns): the packed
    stream is 4.30 GB and the values plane 4.295 GB, both past 2^32 bytes. Values are drawn on
    the device; the first and the last record, the ones around the 2^32-byte crossings of the
    stream and of the plane and every 4 099th are compared on the device, pack and then unpack
    of the packed stream, with a poison word on each side of every output."""
    from distml_amd import DataDesc, pack_push_device, unpack_fetch_device
    n, cols, key_lo = 1_048_700, 1024, -5
    rec = 4 + 4 * cols
    assert n * rec > 1 << 32 and n * 4 * cols > 1 << 32
    fmt = DataDesc(1, 0, 1)
    g = torch.Generator(device="cuda").manual_seed(3)
    vals = torch.randint(-(1 << 31), (1 << 31) - 1, (n, cols), dtype=torch.int32, device="cuda", generator=g)
    P = geom.poison_i32()
    out = torch.full((n * (1 + cols) + 2,), P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cross = {(1 << 32) // rec, (1 << 32) // (4 * cols)}
    idx = sorted({0, n - 1, *range(0, n, 4099)} | {c + d for c in cross for d in (-1, 0, 1)})
    sel = torch.tensor(idx, dtype=torch.int64, device="cuda")
    assert pack_push_device(fmt, cols, key_lo, vals.data_ptr(), n, out.data_ptr() + 4, 4 * (out.numel() - 2)) == n * rec
    assert int(out[0]) == P and int(out[-1]) == P
    r = out[1:-1].view(n, 1 + cols)
    assert torch.equal(r[sel, 0], (sel + key_lo).to(torch.int32))
    assert torch.equal(r[sel, 1:], vals[sel])
    back = torch.full((n * cols + 2,), P, dtype=torch.int32, device="cuda")
    keys = torch.full((n + 2,), geom.poison_i64(), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    unpack_fetch_device(fmt, cols, out.data_ptr() + 4, n, back.data_ptr() + 4, None, keys.data_ptr() + 8)
    assert int(back[0]) == P and int(back[-1]) == P
    assert int(keys[0]) == geom.poison_i64() and int(keys[-1]) == geom.poison_i64()
    assert torch.equal(back[1:-1].view(n, cols)[sel], vals[sel])
    assert torch.equal(keys[1:-1][sel], sel + key_lo)
    assert torch.equal(keys[1:-1], torch.arange(key_lo, key_lo + n, dtype=torch.int64, device="cuda"))
    del vals, out, back, keys, r
    torch.cuda.empty_cache()


def raw_pack(fmt, cols, flags, keys_ptr, key_lo, n, values_ptr, out_ptr, cap, stream=None, out_len=True):
    from distml_amd import _lib
    ln = C.c_int64(-7)
    rc = _lib.load().dml_records_pack_device(C.byref(fmt.to_c()) if fmt is not None else None, cols, flags,
                                             C.c_void_p(keys_ptr or None), key_lo, n, C.c_void_p(values_ptr or None),
                                             C.c_void_p(out_ptr or None), cap, C.byref(ln) if out_len else None,
                                             C.c_void_p(stream or None))
    return rc, ln.value


def raw_unpack(fmt, cols, flags, rec_ptr, n, keys_ptr, values_ptr, alpha_ptr, stream=None):
    from distml_amd import _lib
    return _lib.load().dml_records_unpack_device(C.byref(fmt.to_c()) if fmt is not None else None, cols, flags,
                                                 C.c_void_p(rec_ptr or None), n, C.c_void_p(keys_ptr or None),
                                                 C.c_void_p(values_ptr or None), C.c_void_p(alpha_ptr or None),
                                                 C.c_void_p(stream or None))


def test_refusals(oracle):
    """Test 5. Every argument error of the header, in the synchronous and the stream form: the
    status and *out_len as documented (n x push record bytes once desc, cols, flags and n are
    valid, else 0), and every arena, inputs and outputs, still as uploaded."""
    from distml_amd import DataDesc, _lib
    E, U, CAP, BD = _lib.DML_E_INVALID_ARG, _lib.DML_E_UNSUPPORTED, _lib.DML_E_CAPACITY, _lib.DML_E_BAD_DESC
    case = fc._case("ada", 1, 1, 1, 5, 301, geom.BIG33, True)
    fmt, cols, n = fmt_of(case), 5, 9
    plain = DataDesc(1, 1, 1, False, True, False)
    sparse = DataDesc(1, 1, 1, False, False, False)
    baddesc = DataDesc(1, 1, 2, False, True, False)
    prec, frec = 8 + 4 * cols, 8 + 8 * cols
    full = n * prec
    _, o = fc.make_oracle(case, oracle)
    keys = case["first"] + np.arange(n, dtype=np.int64)
    ka = geom.pack([keys.tobytes()], 0)
    va = geom.pack([cc.pack_values(case, n).tobytes()], 4)
    ra = geom.pack([o.fetch(keys)], 8)
    out = geom.OutArena(full, 4).upload()
    pv, pa, pk = (geom.OutArena(n * cols * 4, 12).upload(), geom.OutArena(n * cols * 4, 4).upload(),
                  geom.OutArena(n * 8, 8).upload())
    K, V, R, O = ka.ptrs[0], va.ptrs[0], ra.ptrs[0], out.ptr
    st = torch.cuda.Stream()
    for stream in (None, st.cuda_stream):
        for what, args, want in (
                ("n -1", (fmt, cols, 0, K, 0, -1, V, O, full), (E, 0)),
                ("null desc", (None, cols, 0, K, 0, n, V, O, full), (E, 0)),
                ("cols 0", (fmt, 0, 0, K, 0, n, V, O, full), (E, 0)),
                ("cols -3", (fmt, -3, 0, K, 0, n, V, O, full), (E, 0)),
                ("flag 0x100", (fmt, cols, 0x100, K, 0, n, V, O, full), (E, 0)),
                ("sparse column", (sparse, cols, 0, K, 0, n, V, O, full), (U, 0)),
                ("bad desc", (baddesc, cols, 0, K, 0, n, V, O, full), (BD, 0)),
                ("null values", (fmt, cols, 0, K, 0, n, 0, O, full), (E, full)),
                ("null out", (fmt, cols, 0, K, 0, n, V, 0, full), (E, full)),
                ("keys + 4", (fmt, cols, 0, K + 4, 0, n, V, O, full), (E, full)),
                ("values + 2", (fmt, cols, 0, K, 0, n, V + 2, O, full), (E, full)),
                ("out + 1", (fmt, cols, 0, K, 0, n, V, O + 1, full), (E, full)),
                ("out + 2, n 0", (fmt, cols, 0, K, 0, 0, V, O + 2, full), (E, 0)),
                ("cap short", (fmt, cols, 0, K, 0, n, V, O, full - 4), (CAP, full)),
                ("cap 0", (fmt, cols, 0, 0, 77, n, V, O, 0), (CAP, full)),
                ("out over values", (fmt, cols, 0, K, 0, n, V, V + n * cols * 4 - 4, full), (E, full)),
                ("out over values' head", (fmt, cols, 0, K, 0, n, V, V - full + 4, full), (E, full)),
                ("out over keys", (fmt, cols, 0, K, 0, n, V, K + 8 * n - 4, full), (E, full))):
            assert raw_pack(*args, stream=stream) == want, what
        assert raw_pack(fmt, cols, 0, K, 0, n, V, O, full, stream=stream, out_len=False)[0] == E
        assert raw_pack(fmt, cols, 0, 0, 0, 0, 0, 0, 0, stream=stream) == (0, 0)  # n == 0: nothing to do
        for what, args, want in (
                ("n -1", (fmt, cols, 0, R, -1, pk.ptr, pv.ptr, pa.ptr), E),
                ("null desc", (None, cols, 0, R, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("cols 0", (fmt, 0, 0, R, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("flag 0x8", (fmt, cols, 0x8, R, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("sparse column", (sparse, cols, 0, R, n, pk.ptr, pv.ptr, 0), U),
                ("bad desc", (baddesc, cols, 0, R, n, pk.ptr, pv.ptr, 0), BD),
                ("no plane", (fmt, cols, 0, R, n, 0, 0, 0), E),
                ("alpha, not AdaGrad", (plain, cols, 0, R, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("null records", (fmt, cols, 0, 0, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("records + 2", (fmt, cols, 0, R + 2, n, pk.ptr, pv.ptr, pa.ptr), E),
                ("values + 2", (fmt, cols, 0, R, n, pk.ptr, pv.ptr + 2, pa.ptr), E),
                ("alpha + 1", (fmt, cols, 0, R, n, pk.ptr, pv.ptr, pa.ptr + 1), E),
                ("keys + 4", (fmt, cols, 0, R, n, pk.ptr + 4, pv.ptr, pa.ptr), E),
                ("values over records", (fmt, cols, 0, R, n, pk.ptr, R + n * frec - 4, pa.ptr), E),
                ("alpha over records", (fmt, cols, 0, R, n, pk.ptr, pv.ptr, R - n * cols * 4 + 4), E),
                ("keys over records", (fmt, cols, 0, R, n, R + 8, pv.ptr, pa.ptr), E),
                ("alpha over values", (fmt, cols, 0, R, n, pk.ptr, pv.ptr, pv.ptr + 8), E)):
            assert raw_unpack(*args, stream=stream) == want, what
        assert raw_unpack(fmt, cols, 0, 0, 0, pk.ptr, pv.ptr, pa.ptr, stream=stream) == 0  # n == 0
    st.synchronize()
    for a in (out, pv, pa, pk):
        a.read()
        a.untouched([])
    for a in (ka, va, ra):
        a.check()
    # and the same arguments, in order, work
    assert raw_pack(fmt, cols, 0, K, 0, n, V, O, full) == (0, full)
    assert raw_unpack(fmt, cols, 0, R, n, pk.ptr, pv.ptr, pa.ptr) == 0


@pytest.mark.parametrize("case", [fc._case("f32", 1, 0, 1, 50, 301, geom.NEG32),
                                  fc._case("af32ref", 0, 1, 1, 1, 1237, geom.BIG33, False, True)], ids=lambda c: c["id"])
def test_stream_form(case):
    """Test 6. On one caller stream with no host wait in between: a torch op that produces the
    values, pack, unpack of the packed records (the push layout of these stores is a fetch
    layout). One synchronise at the end; packed bytes and planes are the host codec's."""
    from distml_amd import pack_push_device, unpack_fetch_device
    n, cols = 4099, case["cols"]
    rec = cc.push_record_bytes(case)
    assert rec == fc.record_bytes(case)
    fmt = fmt_of(case)
    rng = np.random.default_rng(12)
    a = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32)).cuda()
    b = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32)).cuda()
    out = geom.OutArena(n * rec, 12).upload()
    pv, pk = geom.OutArena(n * cols * 4, 4).upload(), geom.OutArena(n * 8, 8).upload()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for _ in range(20):  # enough work ahead of the pack that it would run early if it did not queue
            b = b * 1.0001 + a
        grad = (a * 0.5 - b).contiguous()
        assert pack_push_device(fmt, cols, -7, grad.data_ptr(), n, out.ptr, n * rec, stream=st.cuda_stream,
                                flags=cc.flags(case)) == n * rec
        unpack_fetch_device(fmt, cols, out.ptr, n, pv.ptr, None, pk.ptr, stream=st.cuda_stream, flags=cc.flags(case))
    st.synchronize()
    g = grad.cpu().numpy()
    keys = -7 + np.arange(n, dtype=np.int64)
    same(out.read(), cc.pack_expected(case, keys, g), "stream pack")
    out.untouched([(0, n * rec)])
    same(pv.read(), g.tobytes(), "stream values")
    pv.untouched([(0, n * cols * 4)])
    same(pk.read(), keys.tobytes(), "stream keys")
    pk.untouched([(0, n * 8)])

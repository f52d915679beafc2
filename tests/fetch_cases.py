"""The case table of tests/test_gpu_fetch_device.py: stores, initial values, key lists and
ranges of the device fetch (dml_store_fetch_device), and the oracle set up the same way.

Pure numpy plus the CPU oracle: tests/test_fetch_device_cases.py pins the table without a
GPU (record sizes cover the four residues mod 16, every store class is present, the
oracle's fetch of a list is the concatenation of its single-key fetches, the out-of-shard
plan puts the lower index on first - 1).
"""
import zlib

import numpy as np

import geom

WIDTHS = (1, 3, 4, 5, 17, 50, 200, 256, 1000, 1023, 1025)
# (tag, value type, AdaGrad): FloatMatrixStore, IntMatrixStore, DoubleMatrixStore, FloatMatrixStoreAdaGrad
MATRIX_STORES = (("f32", 1, False), ("i32", 0, False), ("f64", 3, False), ("ada", 1, True))
# (tag, value type, DML_FLAG_FLOAT_ARRAY_REF_STRIDE): IntArrayStore, FloatArrayStore (twice), DoubleArrayStore
ARRAY_STORES = (("ai32", 0, False), ("af32", 1, False), ("af32ref", 1, True), ("af64", 3, False))
FIRST64 = (1000, geom.BIG33, geom.STRADDLE)
FIRST32 = (1000, geom.NEG32)
ADA = geom.ADA
VDT = {0: np.int32, 1: np.float32, 3: np.float64}


def _case(tag, dt, kt, vt, cols, rows, first, ada=False, ref_stride=False):
    return dict(id=f"{tag}-c{cols}-k{4 + 4 * kt}-first{first}", dt=dt, kt=kt, vt=vt, cols=cols, rows=rows,
                first=first, ada=ada, ref_stride=ref_stride, store=tag)


def _cases():
    out, n = [], 0
    for tag, vt, ada in MATRIX_STORES:
        for cols in WIDTHS:
            kt = n % 2  # key types alternate down the table; every store meets both at every residue class
            firsts = FIRST64 if kt else FIRST32
            out.append(_case(tag, 1, kt, vt, cols, 301 if cols >= 256 else 1237, firsts[(n // 2) % len(firsts)], ada))
            n += 1
        n += 1  # shift the alternation: the next store starts on the other key type
    for tag, vt, ref in ARRAY_STORES:
        for kt in (0, 1):
            firsts = FIRST64 if kt else FIRST32
            out.append(_case(tag, 0, kt, vt, 1, 1237, firsts[n % len(firsts)], False, ref))
            n += 1
    return out


CASES = _cases()


def record_bytes(case):
    """Bytes of one fetched record (handleFetch, dense column)."""
    K = 4 + 4 * case["kt"]
    V = 8 if case["vt"] == 3 else 4
    if case["dt"] == 1:
        return K + case["cols"] * (8 if case["ada"] else V)
    return K + (8 if case["vt"] == 1 else V)  # FloatArrayStore's 8-byte slot


def specials(vt):
    """Bit patterns that any float arithmetic, flush-to-zero or canonicalisation would
    change: -0.0, denormals, +-Inf, quiet NaNs with distinct payloads (as raw words)."""
    if vt == 1:
        return np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345,
                         0x7FFABCDE], "<u4")
    if vt == 3:
        return np.array([0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000,
                         0xFFF0000000000000, 0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FFDEADBEEF00001], "<u8")
    return np.array([0x80000000, 0x7FFFFFFF, 0xFFFFFFFF, 0], "<u4")  # INT_MIN, INT_MAX, -1, 0


def build_init(case, plain=False):
    """rows x cols initial values. Specials are sprinkled over the odd rows; `plain` leaves
    them out (the round trip adds the values to zero). AdaGrad cases push the even rows
    afterwards, so no special meets arithmetic."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    rows, cols, vt = case["rows"], case["cols"], case["vt"]
    if vt == 0:
        a = rng.integers(-(1 << 31), 1 << 31, size=(rows, cols)).astype(np.int32)
    else:
        a = rng.standard_normal((rows, cols)).astype(VDT[vt])
    if not plain:
        sp = specials(vt)
        raw = a.view(sp.dtype)
        odd = np.arange(1, rows, 2)
        for i, r in enumerate(rng.choice(odd, size=min(len(odd), 4 * len(sp)), replace=False)):
            raw[r, rng.integers(0, cols)] = sp[i % len(sp)]
        if not case["ada"]:  # and on the shard's corners, where no push follows
            raw[0, 0] = sp[0]
            raw[rows - 1, cols - 1] = sp[1]
    return a


def ada_push(case):
    """The one push of an AdaGrad case: every even row, so alpha and delta vary by row."""
    from distml_amd.store import encode_matrix_push
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()) + 1)
    r = np.arange(0, case["rows"], 2)
    v = (rng.standard_normal((len(r), case["cols"])) * 0.6).astype(np.float32)
    return encode_matrix_push(case["first"] + r.astype(np.int64), v, case["kt"], case["vt"])


def make_oracle(case, pyoracle, init=None):
    """(init, oracle store) of a case: init loaded, AdaGrad cases after setAlpha and ada_push."""
    init = build_init(case) if init is None else init
    o = pyoracle.OracleStore(case["dt"], case["kt"], case["vt"], case["first"], case["first"] + case["rows"] - 1,
                             case["cols"], 1, int(case["ada"]), int(case["ref_stride"]))
    if case["ada"]:
        o.set_alpha(*ADA)
    o.data[:] = init
    if case["ada"]:
        assert o.push(ada_push(case)) == 0
    return init, o


def key_lists(case):
    """name -> int64 keys: every row ascending; a shuffled subset with repeats that holds the
    shard's first and last key; one key; no key."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()) + 2)
    first, rows = case["first"], case["rows"]
    sub = rng.choice(rows, size=rows // 3, replace=False)
    sub = np.concatenate([sub, sub[:37], [0, rows - 1, rows - 1]])
    rng.shuffle(sub)
    return {"asc": first + np.arange(rows, dtype=np.int64),
            "shuffled": first + sub.astype(np.int64),
            "one": np.array([first + rows // 2], np.int64),
            "none": np.zeros(0, np.int64)}


def ranges(case):
    """name -> (requested first, requested last, the keys the fetch returns)."""
    first, rows = case["first"], case["rows"]
    last = first + rows - 1
    ar = lambda a, b: np.arange(a, b + 1, dtype=np.int64)  # noqa: E731
    return {"whole": (first, last, ar(first, last)),
            "clipped": (first - 5, last + 9, ar(first, last)),       # sticks out on both sides
            "inner": (first + 2, last - 3, ar(first + 2, last - 3)),
            "left": (first - 5, first + 6, ar(first, first + 6)),     # clipped on one side
            "one": (first + 7, first + 7, ar(first + 7, first + 7)),
            "disjoint": (last + 10, last + 20, np.zeros(0, np.int64))}


def out_of_shard_plan(case, n=12):
    """Test 6's list: n in-shard keys, then last + 1 at index 7 and first - 1 at index 3.
    Returns (keys, indices of the refused records, the key the store reports)."""
    first, last = case["first"], case["first"] + case["rows"] - 1
    keys = first + np.arange(n, dtype=np.int64) * 3
    keys[7] = last + 1
    keys[3] = first - 1
    return keys, (3, 7), first - 1


# Tiling edges (test 2): f32 rows of 5 columns behind int32 keys, 24-byte records. Whole
# wave runs (1 024 B) end on a record every 3 072 B = 128 records, whole blocks (4 096 B)
# every 12 288 B = 512 records.
EDGE_CASE = _case("f32", 1, 0, 1, 5, 2100, 1000)


def edge_counts(wave_bytes, block_bytes):
    rec = record_bytes(EDGE_CASE)
    out = []
    for unit, whole in ((wave_bytes, 3), (block_bytes, 1)):
        per = np.lcm(rec, unit) // rec  # records until a record end meets a tile end again
        n = per * whole
        assert (n * rec) % unit == 0
        out += [n - 1, n, n + 1]
    return out

"""The case table of tests/test_gpu_codec.py and the numpy expectations of the device record
codec (dml_records_pack_device / dml_records_unpack_device).

The stores are fetch_cases.CASES: the four matrix stores at 1 ... 1025 columns, the three
array stores, FloatArrayStore under DML_FLAG_FLOAT_ARRAY_REF_STRIDE, both key types, first
keys beyond 2^32 and below zero. pack-expected is the host encoder (encode_matrix_push /
encode_array_push); unpack-expected is a structured-dtype view of the bytes the CPU oracle's
fetch returns. Pure numpy plus the oracle: tests/test_codec_cases.py pins all of it without
a GPU.
"""
import zlib

import numpy as np

import fetch_cases as fc

CASES = fc.CASES
REF_STRIDE = 0x1  # DML_FLAG_FLOAT_ARRAY_REF_STRIDE


def flags(case):
    return REF_STRIDE if case["ref_stride"] else 0


def key_bytes(case):
    return 4 + 4 * case["kt"]


def value_bytes(case):
    return 8 if case["vt"] == 3 else 4


def push_record_bytes(case):
    """Bytes of one push record (SparseMatrix.writeMap / SparseArray.writeMap)."""
    if case["dt"] == 1:
        return key_bytes(case) + case["cols"] * value_bytes(case)
    return key_bytes(case) + (8 if case["ref_stride"] else value_bytes(case))


def same_layout(case):
    """The fetched record is byte for byte a push record."""
    return push_record_bytes(case) == fc.record_bytes(case) and not case["ada"]


def pack_values(case, n, seed=0):
    """n x cols values of the case's type, with -0.0, denormals, +-Inf and NaN payloads (the
    ints: INT_MIN, INT_MAX, -1, 0) sprinkled over them; every one of them when there is room."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()) + 17 + seed)
    cols, vt = case["cols"], case["vt"]
    if vt == 0:
        a = rng.integers(-(1 << 31), 1 << 31, size=(n, cols)).astype(np.int32)
    else:
        a = rng.standard_normal((n, cols)).astype(fc.VDT[vt])
    sp = fc.specials(vt)
    raw = a.view(sp.dtype).reshape(-1)
    if raw.size:
        at = rng.choice(raw.size, size=min(raw.size, 3 * len(sp)), replace=False)
        raw[at] = sp[np.arange(len(at)) % len(sp)]
    return a


def pack_expected(case, keys, values):
    """The host encoder's bytes for these keys (int64) and values (n x cols)."""
    from distml_amd.store import encode_array_push, encode_matrix_push
    keys = np.asarray(keys, np.int64)
    if case["dt"] == 1:
        return encode_matrix_push(keys, values.reshape(len(keys), case["cols"]), case["kt"], case["vt"])
    return encode_array_push(keys, values.reshape(-1), case["kt"], case["vt"], 8 if case["ref_stride"] else None)


def fetch_dtype(case):
    """One fetched record as a structured dtype (handleFetch, dense column)."""
    k = ("k", "<i4" if case["kt"] == 0 else "<i8")
    v = np.dtype(fc.VDT[case["vt"]]).newbyteorder("<")
    if case["ada"]:
        return np.dtype([k, ("s", [("v", "<f4"), ("a", "<f4")], (case["cols"],))])
    if case["dt"] == 0 and case["vt"] == 1:
        return np.dtype([k, ("v", "<f4", (1,)), ("pad", "<u4")])  # FloatArrayStore's 8-byte slot
    return np.dtype([k, ("v", v, (case["cols"],))])


def unpack_expected(case, fetched):
    """(keys int64[n], values T[n][cols], alpha f32[n][cols] or None) of fetched bytes."""
    r = np.frombuffer(fetched, fetch_dtype(case))
    assert r.nbytes == len(fetched) and r.dtype.itemsize == fc.record_bytes(case)
    keys = r["k"].astype(np.int64)  # int32 keys sign-extend (DataDesc.readKey)
    if case["ada"]:
        return keys, np.ascontiguousarray(r["s"]["v"]), np.ascontiguousarray(r["s"]["a"])
    return keys, np.ascontiguousarray(r["v"]).reshape(len(r), case["cols"]), None


def wire_key(case, keys):
    """The keys as a record holds them and a reader sees them again: an int32 key is the low
    four bytes of the int64, sign-extended on the way back."""
    keys = np.asarray(keys, np.int64)
    return keys if case["kt"] == 1 else keys.astype("<i4").astype(np.int64)


def pack_key_lists(case):
    """name -> int64 keys of the pack's list form: shuffled with repeats, one key, no key.
    Pack refuses no key, so they are not tied to a shard: int64 cases carry keys beyond 2^32
    and negative ones, int32 cases keys whose high word is set (cut off by the writer)."""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()) + 5)
    n = 41 if case["cols"] >= 256 else 173
    base = case["first"] + rng.choice(5000, size=n - 9, replace=False).astype(np.int64)
    keys = np.concatenate([base, base[:5], [case["first"], -3, (1 << 40) + 11, -(1 << 35) + 2]])
    rng.shuffle(keys)
    return {"shuffled": keys, "one": keys[:1].copy(), "none": np.zeros(0, np.int64)}


# Tiling edges: 24-byte records (5 f32 columns, int32 keys; fetch_cases.EDGE_CASE) and 12-byte
# array records (f64 values behind int32 keys).
EDGE_CASE = fc.EDGE_CASE
EDGE_ARRAY = fc._case("af64", 0, 0, 3, 1, 2100, 1000)


def edge_counts(unit_bytes, wave_bytes, block_bytes):
    """Counts n at which a run of n x unit_bytes ends one unit before, at and one unit past
    three whole wave runs and one whole block: fetch_cases.edge_counts for any unit (a push
    record for pack's stream, cols x V for unpack's values plane)."""
    out = []
    for tile, whole in ((wave_bytes, 3), (block_bytes, 1)):
        per = int(np.lcm(unit_bytes, tile)) // unit_bytes
        n = per * whole
        assert (n * unit_bytes) % tile == 0
        out += [n - 1, n, n + 1]
    return out

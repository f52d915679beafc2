"""The numpy model of dml_coalesce_device, and the inputs its tests share.

`coalesce(keys, values)` is the contract of include/distml_ps.h read literally: the distinct
keys ascending as signed 64-bit values (np.unique), each occurrence's place among them
(return_inverse), and per key the sum of its rows from +0.0, one add per occurrence IN LIST
ORDER, each add rounded once in the value's own type; int32 adds go through uint32, so they
wrap. tests/test_coalesce_expect.py pins the model to the CPU oracle (a zero store after one
push of the occurrences) and shows that it tells summation orders apart; the GPU tests
compare bytes with it.

Pure numpy, but for raw_call and refusal_cases at the end, which bind the library.
"""
import ctypes as C

import numpy as np

VDT = {0: np.int32, 1: np.float32, 3: np.float64}
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def coalesce(keys, values=None):
    """(unique keys int64[m], inverse int32[n], sums T[m][cols] or None)."""
    keys = np.ascontiguousarray(keys, dtype=np.int64)
    uk, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(-1).astype(np.int32)
    if values is None:
        return uk, inv, None
    v = np.ascontiguousarray(values)
    v = v.reshape(len(keys), -1)
    acc = v.view(np.uint32) if v.dtype == np.int32 else v
    out = np.zeros((len(uk), acc.shape[1]), acc.dtype)  # +0.0
    with np.errstate(all="ignore"):
        for j in range(len(keys)):  # list order; one rounding per add
            out[inv[j]] = out[inv[j]] + acc[j]
    return uk, inv, out.view(v.dtype)


# ------------------------------------------------------------------ key patterns
def skewed(first, depth, batch, seed=0):
    """Keys whose segments have exactly depth - 1, depth + 1, batch - 1, batch, batch + 1
    and 2 x batch + 1 occurrences, each next to keys that occur once, in a shuffled list
    order (so a segment's occurrences are spread over the list)."""
    lens = [depth - 1, depth + 1, batch - 1, batch, batch + 1, 2 * batch + 1]
    ks = []
    for i, ln in enumerate(lens):
        ks += [first + 3 * i] * ln + [first + 3 * i + 1]  # a long segment, then a segment of 1
    ks += [first - 5, first + 3 * len(lens) + 7]
    ks = np.array(ks, np.int64)
    return ks[np.random.default_rng(seed).permutation(len(ks))]


def patterns(first, n, depth, batch, seed=0):
    """name -> int64 key list of about n keys, for one layout."""
    rng = np.random.default_rng(seed)
    return {
        "asc": first + np.arange(n, dtype=np.int64),
        "perm": first + rng.permutation(n).astype(np.int64),
        "equal": np.full(n, first + 11, np.int64),
        "two": first + (np.arange(n, dtype=np.int64) & 1) * 9,
        "skewed": skewed(first, depth, batch, seed),
        "random": first + rng.integers(0, max(2, n // 3), size=n).astype(np.int64),
    }


def heads_straddle(block_keys, first=1000, seed=0):
    """A list whose sorted order has one key's run of 7 over positions block_keys - 3 ..
    block_keys + 3 (it straddles the first block boundary of k_co_heads)."""
    ks = [first + i for i in range(block_keys - 3)] + [first + block_keys] * 7 + \
         [first + block_keys + 1 + i for i in range(20)]
    ks = np.array(ks, np.int64)
    return ks[np.random.default_rng(seed).permutation(len(ks))]


def heads_at_boundary(block_keys, first=1000, seed=0):
    """... and one whose run of 5 starts exactly at sorted position block_keys."""
    ks = [first + i for i in range(block_keys)] + [first + block_keys] * 5 + [first + block_keys + 9] * 2
    ks = np.array(ks, np.int64)
    return ks[np.random.default_rng(seed).permutation(len(ks))]


# ------------------------------------------------------------------ values
def values(vt, n, cols, seed=0, scale=1.0):
    """n x cols values: floats with magnitudes over 1e-3 .. 1e3 (so that the order of the
    adds decides low bits), int32 counters in [-3, 3]."""
    rng = np.random.default_rng(seed)
    if vt == 0:
        return rng.integers(-3, 4, size=(n, cols)).astype(np.int32)
    mag = 10.0 ** rng.uniform(-3, 3, size=(n, cols))
    return (rng.standard_normal((n, cols)) * mag * scale).astype(VDT[vt])


def special_case(vt):
    """(keys, values n x 4) for the value edge cases, one column each where it matters:
    key 1 a lone -0.0; key 2 -0.0 twice; key 3 -0.0 then +1; key 4 a NaN payload among
    numbers (one NaN per sum: which of two NaNs an add returns is not IEEE's to say); key 5
    +Inf then -Inf (the invalid operation's NaN is x86-64's negative one, on the CPU and,
    by the header's contract, on the device); key 6 denormals; key 7 2^24 (2^53), 1, 1; key 8 1, 1, 2^24 (2^53): ties
    to even, where the order decides the last bit; int32: INT_MAX + 1 and a wrap back."""
    if vt == 0:
        keys = np.array([1, 1, 2, 2, 2, 3], np.int64)
        v = np.array([[0x7FFFFFFF, 5, -7, 0], [1, -9, 7, 0], [-(1 << 31), 1, 2, 3], [-1, 1, 2, 3],
                      [1 << 30, 1, 2, 3], [-(1 << 31), 0, 0, 0]], np.int32)
        return keys, v
    dt = VDT[vt]
    u = np.uint32 if vt == 1 else np.uint64
    big = dt(2.0 ** 24 if vt == 1 else 2.0 ** 53)
    nan = np.array([0x7FC12345 if vt == 1 else 0x7FF8123456789ABC], u).view(dt)[0]
    snan = np.array([0x7FA00001 if vt == 1 else 0x7FF4000000000001], u).view(dt)[0]
    den = np.array([1], u).view(dt)[0]
    den2 = np.array([0x007FFFFF if vt == 1 else 0x000FFFFFFFFFFFFF], u).view(dt)[0]
    inf = dt(np.inf)
    rows = [
        (1, [-0.0, -0.0, 1.5, -0.0]),
        (2, [-0.0, 0.0, -0.0, 2.0]), (2, [-0.0, -0.0, 0.0, -2.0]),
        (3, [-0.0, 1.0, -1.0, 0.0]), (3, [1.0, -1.0, -0.0, -0.0]),
        (4, [1.0, nan, 3.0, snan]), (4, [nan, 2.0, 4.0, 0.0]), (4, [2.0, 3.0, nan, 1.0]),
        (5, [inf, -inf, inf, 1.0]), (5, [-inf, inf, inf, inf]),
        (6, [den, -den, den2, den]), (6, [den, den, den, -den2]), (6, [-den, den2, -den2, den]),
        (7, [big, big, 1.0, 1.0]), (7, [1.0, 1.0, 1.0, big]), (7, [1.0, 1.0, big, 1.0]),
        (8, [1.0, 1.0, big, 1.0]), (8, [1.0, 1.0, 1.0, 1.0]), (8, [big, big, 1.0, big]),
    ]
    keys = np.array([k for k, _ in rows], np.int64)
    v = np.array([r for _, r in rows], dt)
    v.view(u)[5, 3] = snan.view(u)  # as raw bits: a conversion on the way would quiet it
    return keys, v


# ------------------------------------------------------------------ the raw call and its refusals
def raw_call(L, c, fmt, cols, keys, n, values, keys_out, values_out, inverse, cap, out_rows=True, stream=None):
    m = C.c_int64(-7)
    rc = L.dml_coalesce_device(C.c_void_p(c or None), C.byref(fmt.to_c()) if fmt is not None else None, cols,
                               C.c_void_p(keys or None), n, C.c_void_p(values or None), C.c_void_p(keys_out or None),
                               C.c_void_p(values_out or None), C.c_void_p(inverse or None), cap,
                               C.byref(m) if out_rows else None, C.c_void_p(stream or None))
    return rc, m.value


def refusal_cases(K, V, KO, VO, IO, n, cols):
    """(what, arguments after the context, status): every DML_E_INVALID_ARG / _BAD_DESC /
    _UNSUPPORTED case of the header. K .. IO are addresses (never dereferenced by a refusal):
    keys, values, keys out, values out, inverse, far enough apart for n rows of 4 x cols bytes."""
    from distml_amd import DataDesc, _lib
    E, U, BD = _lib.DML_E_INVALID_ARG, _lib.DML_E_UNSUPPORTED, _lib.DML_E_BAD_DESC
    fmt = DataDesc(1, 1, 1, False, True, False)
    arr = DataDesc(0, 1, 1, False, True, False)
    sparse = DataDesc(1, 1, 1, False, False, False)
    baddesc = DataDesc(1, 1, 2, False, True, False)
    row = 4 * cols
    return [
        ("null desc", (None, cols, K, n, V, KO, VO, IO, n), E),
        ("n -1", (fmt, cols, K, -1, V, KO, VO, IO, n), E),
        ("cols 0", (fmt, 0, K, n, V, KO, VO, IO, n), E),
        ("cols -3", (fmt, -3, K, n, V, KO, VO, IO, n), E),
        ("null keys", (fmt, cols, 0, n, V, KO, VO, IO, n), E),
        ("null keys out", (fmt, cols, K, n, V, 0, VO, IO, n), E),
        ("values without values out", (fmt, cols, K, n, V, KO, 0, IO, n), E),
        ("values out without values", (fmt, cols, K, n, 0, KO, VO, IO, n), E),
        ("values out without values, n 0", (fmt, cols, K, 0, 0, KO, VO, IO, n), E),
        ("keys + 4", (fmt, cols, K + 4, n, V, KO, VO, IO, n), E),
        ("keys out + 4", (fmt, cols, K, n, V, KO + 4, VO, IO, n), E),
        ("values + 2", (fmt, cols, K, n, V + 2, KO, VO, IO, n), E),
        ("values out + 1", (fmt, cols, K, n, V, KO, VO + 1, IO, n), E),
        ("inverse + 2", (fmt, cols, K, n, V, KO, VO, IO + 2, n), E),
        ("inverse + 2, n 0", (fmt, cols, K, 0, V, KO, VO, IO + 2, n), E),
        ("keys out over keys", (fmt, cols, K, n, V, K + 8 * n - 8, VO, IO, n), E),
        ("keys out over values", (fmt, cols, K, n, V, V + 8, VO, IO, n), E),
        ("values out over values' tail", (fmt, cols, K, n, V, KO, V + n * row - 4, IO, n), E),
        ("values out over values' head", (fmt, cols, K, n, V, KO, V - n * row + 4, IO, n), E),
        ("values out over keys", (fmt, cols, K, n, V, KO, K + 8, IO, n), E),
        ("inverse over keys", (fmt, cols, K, n, V, KO, VO, K + 8 * n - 4, n), E),
        ("inverse over values", (fmt, cols, K, n, V, KO, VO, V - 4 * n + 4, n), E),
        ("inverse over keys out", (fmt, cols, K, n, V, KO, VO, KO + 8 * n - 4, n), E),
        ("inverse over values out", (fmt, cols, K, n, V, KO, VO, VO + 4, n), E),
        ("values out over keys out", (fmt, cols, K, n, V, KO, KO + 8 * n - 4, IO, n), E),
        ("array: values out over values (cols ignored)", (arr, 0, K, n, V, KO, V + 4 * n - 4, IO, n), E),
        ("bad desc", (baddesc, cols, K, n, V, KO, VO, IO, n), BD),
        ("sparse column", (sparse, cols, K, n, V, KO, VO, IO, n), U),
        ("n 2^31", (fmt, cols, K, 1 << 31, 0, KO, 0, 0, n), U),
        ("row of 2^31 dwords", (DataDesc(1, 1, 3, False, True, False), 1 << 30, K, n, V, KO, VO, IO, n), U),
    ]

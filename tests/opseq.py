"""Seeded operation sequences for one store (pure numpy: no GPU, no torch).

`make_sequence(config, seed)` builds the mixed life of one shard: an init op, then
bursts of 1-4 push calls issued back to back (two chunks in flight, the third call
forces a retire), each burst followed by one sync / read op. Every op is a plain dict
that a runner can apply to the CPU oracle (`OracleSide`, below) and to a `DataStore`
(tests/test_gpu_opseq.py). The generator never looks at a store: a sequence is a
function of (config, seed) alone.

Planned errors: a push call whose `error` is not None makes the reference throw at that
call with exactly that (code, key, col); the calls behind it in the burst carry
`applied = False` (neither side applies them) and the burst's sync op clears the error
on both sides. tests/test_opseq.py checks on the oracle that errors happen there and
nowhere else.

Values. Floats are normals scaled by 2^k, k in [-30, 10] ([-30, 2] for AdaGrad
gradients), with a few -0.0, denormal and +-Inf elements and, on the plain-sum stores,
NaNs. So that no add ever has to choose between two NaNs or create one (x86 and the GPU
choose differently; neither is the store's business): pushed NaNs carry one payload and
go to column 0 only, raw checkpoint bytes never hold a NaN in column 0, +Inf goes to
even element indices and -Inf to odd ones. int32 shards start at 1000-2000 with deltas
in [-2, 3]; only the planned-negative calls use a large negative delta, and the burst's
sync op then rewrites the row (syncFrom), so no later add meets the negative counter.
"""
import hashlib
import zlib

import numpy as np

MATRIX, ARRAY = 1, 0
I32, F32, F64 = 0, 1, 3
E_KEY, E_TRUNC, E_NEG = 2, 3, 4  # DML_E_KEY_OUT_OF_SHARD, DML_E_TRUNCATED, DML_E_NEGATIVE_COUNTER
VDT = {I32: np.int32, F32: np.float32, F64: np.float64}
UDT = {I32: np.uint32, F32: np.uint32, F64: np.uint64}
NAN_BITS = {F32: 0x7FC12345, F64: 0x7FF8000012345678}
ALPHA0 = (0.025, 0.001, 1.5)
SEEDS = (1, 2, 3)
BIG_NEG = -1_000_000
ERROR_KINDS = ("ragged_val", "ragged_key", "oos", "neg_final", "neg_hidden")


def _cfg(name, data_type, key_type, value_type, first, rows, cols=1, ada=False, ref_stride=False, wide=False):
    return dict(name=name, data_type=data_type, key_type=key_type, value_type=value_type, first=first, rows=rows,
                cols=cols, ada=ada, ref_stride=ref_stride, wide=wide)


# The smallest shapes at which each dispatch of launch_chunk / retire_front still happens
# (spec_shape, use_flat, reduce_clears_slots in dml_kernels.hip). `wide`: rows of about
# 4 KiB and more, which skip the 65-70 push call.
CONFIGS = {c["name"]: c for c in [
    _cfg("f32_c1024", MATRIX, 0, F32, 1000, 600, 1024, wide=True),      # whole 4-KiB rows: k_reduce_rows FULL, speculation
    _cfg("f32_c2048", MATRIX, 0, F32, 77, 600, 2048, wide=True),        # 8 KiB: two chunk groups per row
    _cfg("f32_c1280", MATRIX, 0, F32, 500, 600, 1280, wide=True),       # pair-packed loop: never speculates
    _cfg("f32_c200", MATRIX, 0, F32, 100, 2000, 200),                   # k_reduce_flat / k_flat_ident
    _cfg("f32_c256", MATRIX, 0, F32, 4096, 1500, 256),
    _cfg("f32_c37", MATRIX, 0, F32, 31, 3000, 37),                      # generic k_reduce
    _cfg("f32_c3", MATRIX, 0, F32, 9, 3000, 3),                         # below one vector
    _cfg("f64_c512", MATRIX, 1, F64, 123_456, 600, 512, wide=True),     # 4 KiB
    _cfg("f64_c100", MATRIX, 1, F64, (1 << 33) + 12_345, 2000, 100),    # flat; keys do not fit 32 bits
    _cfg("f64_c33", MATRIX, 1, F64, 50, 2500, 33),
    _cfg("i32_c1000", MATRIX, 0, I32, 2000, 600, 1000, wide=True),      # checked adds, rollback
    _cfg("i32_c48", MATRIX, 0, I32, 10, 2000, 48),
    _cfg("i32_c7", MATRIX, 0, I32, 3, 3000, 7),
    _cfg("ada_c200", MATRIX, 0, F32, 50, 2000, 200, ada=True),          # k_ada_flat / k_ada_ident / k_reduce
    _cfg("ada_c48", MATRIX, 0, F32, 600, 2500, 48, ada=True),
    _cfg("ada_c300", MATRIX, 0, F32, 20, 1500, 300, ada=True),          # slot table not cleared
    _cfg("arr_f32", ARRAY, 1, F32, 1000, 50_000),
    _cfg("arr_f32_ref8", ARRAY, 1, F32, 5, 50_000, ref_stride=True),    # the reference's 8-byte value stride
    _cfg("arr_f64", ARRAY, 0, F64, 40, 50_000),
    _cfg("arr_i32", ARRAY, 0, I32, 7, 50_000),
]}
# seeds beyond the three that found a defect (its hand-written case sits in tests/test_gpu_parity.py):
# ada_c48 / 6: a no-op chunk's maxDelta finalize consumed the pending candidate of the chunk before it
FOUND = [("ada_c48", 6)]
CASES = [(name, seed) for name in CONFIGS for seed in SEEDS] + FOUND


# ---- what the store's dispatch does with a shape (restated from dml_kernels.hip) ----------
def _vec(cfg):
    return 2 if cfg["value_type"] == F64 else 4


def _row_bytes(cfg):
    return cfg["cols"] * np.dtype(VDT[cfg["value_type"]]).itemsize


def flat_shaped(cfg):
    """use_flat's shape test: whole vectors, rows under 4 KiB."""
    return cfg["data_type"] == MATRIX and cfg["cols"] % _vec(cfg) == 0 and _row_bytes(cfg) < 4096


def spec_shaped(cfg):
    """run_batch speculates on plain-sum float matrices of the spec_shape widths."""
    if cfg["data_type"] != MATRIX or cfg["ada"] or cfg["value_type"] == I32:
        return False
    return _row_bytes(cfg) % 4096 == 0 or flat_shaped(cfg)


def push_kinds(cfg):
    """The push-call kinds a config's sequences hold (each at least once per sequence)."""
    if cfg["data_type"] == MATRIX:
        kinds = ["perm", "ident", "mixed_full", "swap", "dup", "partial_hi", "partial_lo", "small"]
        if cfg["ada"]:
            kinds += ["ada_big", "ada_tie"]
    else:
        kinds = ["arr", "arr_rep", "skew", "small"]
    if not cfg["wide"]:
        kinds.append("long")
    kinds += ["ragged_val", "ragged_key", "oos"]
    if cfg["value_type"] == I32:
        kinds += ["neg_final", "neg_hidden"]
    return kinds


def sync_kinds(cfg):
    kinds = ["flush", "fetch_list", "fetch_range", "write_all", "sync_to", "sync_from", "read_all", "fill",
             "read_rows"]
    if cfg["ada"]:
        kinds.append("set_alpha")
    return kinds


# ---- k_ident_check's sample (dml_kernels.hip), so a corrupted record can hide from it -----
_M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sampled_positions(b, rows):
    """Record positions k_ident_check reads in push b of a chunk: 32 evenly spaced + 32 hashed."""
    ev = {t * (rows - 1) // 31 for t in range(32)}
    hs = {splitmix64((b << 32) + t) % rows for t in range(32, 64)}
    return ev | hs


# ---- record codec (SparseMatrix.writeMap / SparseArray.writeMap layouts) ------------------
def _kdt(cfg):
    return np.dtype("<i4") if cfg["key_type"] == 0 else np.dtype("<i8")


def record_stride(cfg):
    K = _kdt(cfg).itemsize
    V = np.dtype(VDT[cfg["value_type"]]).itemsize
    if cfg["data_type"] == MATRIX:
        return K + cfg["cols"] * V
    return K + (8 if (cfg["ref_stride"] and cfg["value_type"] == F32) else V)


def encode(cfg, keys, vals):
    """keys: absolute int64 keys; vals: (n, cols). Returns a contiguous uint8 array."""
    keys = np.asarray(keys, np.int64)
    vdt = np.dtype(VDT[cfg["value_type"]]).newbyteorder("<")
    n, K, stride = len(keys), _kdt(cfg).itemsize, record_stride(cfg)
    out = np.zeros((n, stride), np.uint8)
    if n == 0:
        return out.reshape(-1)
    out[:, :K] = keys.astype(_kdt(cfg)).view(np.uint8).reshape(n, K)
    v = np.ascontiguousarray(vals, vdt).reshape(n, -1)
    out[:, K:K + v.shape[1] * vdt.itemsize] = v.view(np.uint8).reshape(n, -1)
    return out.reshape(-1)


# ---- generator ---------------------------------------------------------------------------
class _Ctx:
    def __init__(self, cfg, seed):
        self.cfg = cfg
        self.rng = np.random.default_rng([zlib.crc32(cfg["name"].encode()), seed])
        self.R, self.C, self.vt = cfg["rows"], cfg["cols"], cfg["value_type"]
        self.ties = 0
        self.last_burst = False
        rng = self.rng
        shape = (self.R, self.C)
        if self.vt == I32:
            self.pools = [rng.integers(-2, 4, size=shape).astype(np.int32) for _ in range(3)]
        else:
            hi = 2 if cfg["ada"] else 10
            self.pools = [(rng.standard_normal(shape) * np.exp2(rng.integers(-30, hi + 1, size=shape)))
                          .astype(VDT[self.vt]) for _ in range(3)]
        self.perms = [rng.permutation(self.R) for _ in range(int(rng.integers(3, 5)))]

    # values of n records (rows of a pool from a random offset, times a power of two)
    def vals(self, n):
        rng = self.rng
        pool = self.pools[int(rng.integers(len(self.pools)))]
        v = pool[(int(rng.integers(self.R)) + np.arange(n)) % self.R].copy()
        if self.vt != I32:
            v *= VDT[self.vt](2.0 ** int(rng.integers(-2, 3)))
        return v

    def place_specials(self, rowidx, v):
        """A few -0.0, denormal, +-Inf (by element parity) and NaN (column 0, plain sums) values."""
        rng, cfg = self.rng, self.cfg
        if self.vt == I32 or len(rowidx) == 0 or rng.random() > 0.4:
            return
        tiny = np.finfo(VDT[self.vt]).smallest_subnormal
        for _ in range(int(rng.integers(1, 5))):
            p, c = int(rng.integers(len(rowidx))), int(rng.integers(self.C))
            what = int(rng.integers(4))
            if what == 0:
                v[p, c] = -0.0
            elif what == 1:
                v[p, c] = tiny * int(rng.integers(1, 1000)) * (1 if rng.random() < 0.5 else -1)
            elif what == 2:
                if cfg["ada"] and not self.last_burst:
                    continue  # an Inf gradient makes maxDelta Inf for good: only in the last burst
                v[p, c] = np.inf if (int(rowidx[p]) * self.C + c) % 2 == 0 else -np.inf
            elif not cfg["ada"]:
                v.view(UDT[self.vt])[p, 0] = NAN_BITS[self.vt]

    def nb(self, lo=1, hi=9):
        return int(self.rng.integers(lo, hi + 1))

    def subset(self, m):
        r = self.rng.permutation(self.R)[:m]
        return np.sort(r) if self.rng.random() < 0.3 else r

    def free_positions(self, b, n=2):
        """n record positions of push b (ascending) that k_ident_check does not sample."""
        taken = sampled_positions(b, self.R)
        free = [p for p in range(self.R) if p not in taken]
        at = sorted(int(x) for x in self.rng.choice(len(free), size=n, replace=False))
        return [free[i] for i in at]


def _full_rows(ctx, how):
    if how == "ident":
        return np.arange(ctx.R)
    return ctx.perms[how].copy()


def _matrix_base(ctx, kind, nb, sel=None):
    """Row lists of the nb pushes of a call of this base shape."""
    rng, R = ctx.rng, ctx.R
    if kind == "ident":
        return [np.arange(R) for _ in range(nb)]
    if kind == "perm":
        sel = sel if sel is not None else [int(rng.integers(len(ctx.perms))) for _ in range(nb)]
        return [ctx.perms[s].copy() for s in sel]
    if kind == "mixed_full":
        hows = ["ident" if rng.random() < 0.5 else int(rng.integers(len(ctx.perms))) for _ in range(nb)]
        if nb >= 2:
            hows[0], hows[1] = "ident", int(rng.integers(len(ctx.perms)))
            order = rng.permutation(nb)
            hows = [hows[i] for i in order]
        return [_full_rows(ctx, h) for h in hows]
    if kind == "partial_hi":
        rows = [ctx.subset(int(rng.integers(R // 2 + 1, R + 1))) for _ in range(nb)]
        rows[int(rng.integers(nb))] = ctx.subset(int(rng.integers(R // 2 + 1, R)))  # one is not full-range
        return rows
    if kind == "partial_lo":
        rows = [ctx.subset(int(rng.integers(R // 2 + 1, R + 1))) for _ in range(nb)]
        rows[int(rng.integers(nb))] = ctx.subset(int(rng.integers(3, R // 2)))  # lists under half the rows
        return rows
    if kind == "long":
        return [ctx.subset(int(rng.integers(R // 10, R // 4))) for _ in range(nb)]
    raise KeyError(kind)


def _array_base(ctx, kind, nb):
    rng, R = ctx.rng, ctx.R
    if kind == "arr":
        return [rng.permutation(R)[:int(rng.integers(5_000, 20_001))] for _ in range(nb)]
    if kind == "arr_rep":  # ~2-6 repeats of every key inside one push
        return [int(rng.integers(R - 3_000)) + rng.integers(0, 3_000, size=int(rng.integers(5_000, 20_001)))
                for _ in range(nb)]
    if kind == "skew":  # 6000 records on 64 keys: more than a leaf sorts in LDS (2048)
        out = []
        for _ in range(nb):
            hot = int(rng.integers(R - 64)) + rng.integers(0, 64, size=6_000)
            out.append(rng.permutation(np.concatenate([hot, rng.permutation(R)[:5_000]])))
        return out
    if kind == "long":
        return [rng.permutation(R)[:int(rng.integers(300, 801))] for _ in range(nb)]
    raise KeyError(kind)


def _gen_call(ctx, kind, sel=None, nb=None):
    """One push call: {"op": "push", "kind", "pushes": [uint8 arrays], "error", "expects", ...}."""
    cfg, rng, R, C = ctx.cfg, ctx.rng, ctx.R, ctx.C
    matrix = cfg["data_type"] == MATRIX
    first, last = cfg["first"], cfg["first"] + R - 1
    stride, K = record_stride(cfg), _kdt(cfg).itemsize
    V = np.dtype(VDT[ctx.vt]).itemsize
    error, expects, bad_row, cut = None, [], None, {}
    ada_flat = cfg["ada"] and flat_shaped(cfg)

    # ---- the rows each push lists
    if kind == "small":
        nb = nb or ctx.nb(3, 9)
        base = _matrix_base(ctx, "partial_hi", nb) if matrix else _array_base(ctx, "arr", nb)
        e, s = (int(x) for x in rng.choice(nb, size=2, replace=False))
        base[e] = np.zeros(0, np.int64)
        base[s] = rng.integers(0, R, size=1)
    elif kind == "long":
        nb = nb or ctx.nb(65, 70)
        base = _matrix_base(ctx, "long", nb) if matrix else _array_base(ctx, "long", nb)
    elif not matrix:
        nb = nb or ctx.nb()
        shape = kind if kind in ("arr", "arr_rep", "skew") else ("arr" if rng.random() < 0.6 else "arr_rep")
        base = _array_base(ctx, shape, nb)
    else:
        if kind in ("perm", "ident") and ada_flat:
            nb = nb or ctx.nb(1, 4)   # k_ada_flat / k_ada_ident take calls of <= 4 pushes
        elif kind == "mixed_full" and ada_flat:
            nb = nb or ctx.nb(5, 9)   # k_reduce
        nb = nb or ctx.nb(2 if kind in ("swap", "mixed_full", "ada_tie") else 1)
        if kind in ("perm", "ident", "mixed_full", "partial_hi", "partial_lo"):
            shape = kind
        elif kind in ("swap", "dup"):
            shape = "mixed_full"
        elif kind == "oos":
            shape = ("ident", "mixed_full", "partial_hi")[int(rng.integers(3))]
        else:
            shape = ("mixed_full", "partial_hi", "partial_lo")[int(rng.integers(3))]
        base = _matrix_base(ctx, shape, nb, sel)
        if shape in ("perm", "ident", "mixed_full") and spec_shaped(cfg) and kind not in ("ragged_val", "ragged_key"):
            expects.append("spec")
        if kind in ("ident", "mixed_full") and spec_shaped(cfg):
            expects.append("identity")
        if kind == "ident" and spec_shaped(cfg) and flat_shaped(cfg):
            expects.append("ident_launch")
        if kind == "ident" and ada_flat:
            expects.append("k_ada_ident")
        if kind == "perm" and ada_flat:
            expects.append("k_ada_flat")
    if kind == "skew":
        expects.append("sparse_skew")
    rows = [np.asarray(r, np.int64).copy() for r in base]
    vals = [ctx.vals(len(r)) for r in rows]

    # ---- what makes the call its kind
    j = int(rng.integers(nb))
    if kind == "swap":
        # an ascending push with two records swapped where the sample cannot see them: the
        # speculative chunk fails its verification and re-runs; and one relative to a pool order
        rows[j] = np.arange(R)
        a, b = ctx.free_positions(j)
        rows[j][[a, b]] = rows[j][[b, a]]
        k2 = (j + 1) % nb
        rows[k2] = ctx.perms[int(rng.integers(len(ctx.perms)))].copy()
        a, b = ctx.free_positions(k2)
        rows[k2][[a, b]] = rows[k2][[b, a]]
        if spec_shaped(cfg):
            expects.append("rerun")
    elif kind == "dup":
        a, b = ctx.free_positions(j)
        rows[j][b] = rows[j][a]  # one row twice, one missing: the replay path
    elif kind == "oos":
        while len(rows[j]) < 3:
            j = (j + 1) % nb
        p = len(rows[j]) // 2
        bad = last + 7 if rng.random() < 0.5 else first - 3
        rows[j][p] = bad - first
        error = (E_KEY, bad, -1)
    elif kind in ("ragged_val", "ragged_key"):
        while len(rows[j]) < 3:
            j = (j + 1) % nb
        r = int(rng.integers(1, len(rows[j])))
        if kind == "ragged_key":
            cut[j] = r * stride + int(rng.integers(1, K))
            error = (E_TRUNC, 0, -1)
        elif matrix:
            nv = int(rng.integers(0, C))
            cut[j] = r * stride + K + nv * V + int(rng.integers(1, V))
            error = (E_TRUNC, first + int(rows[j][r]), nv)
        else:
            cut[j] = r * stride + K + int(rng.integers(1, min(V, 4) if ctx.vt != F64 else 8))
            error = (E_TRUNC, first + int(rows[j][r]), -1)
    elif kind in ("neg_final", "neg_hidden"):
        while len(rows[j]) < 3:
            j = (j + 1) % nb
        n = len(rows[j])
        p1 = int(rng.integers(0, n - 1))
        c = int(rng.integers(C))
        vals[j][p1, c] = BIG_NEG
        if kind == "neg_hidden":  # a later add of the same push would lift the counter again
            p2 = int(rng.integers(p1 + 1, n))
            rows[j][p2] = rows[j][p1]
            vals[j][p2, c] = -BIG_NEG
        bad_row = int(rows[j][p1])
        error = (E_NEG, first + bad_row, c if matrix else -1)
    elif kind == "ada_big":
        # delta = 4096: alpha = 0.025 / (1.5 * 64) < minAlpha = 0.001
        for _ in range(int(rng.integers(2, 9))):
            vals[j][int(rng.integers(len(rows[j]))), int(rng.integers(C))] = 64.0 * (1 if rng.random() < 0.5 else -1)
    elif kind == "ada_tie":
        # the same delta 2^(48 + 2t) at two elements (half an ulp there is above any delta the
        # other gradients add up to): the reference's strict > keeps the first
        g = np.float32(2.0 ** (24 + ctx.ties))
        ctx.ties += 1
        j1, j2 = sorted(int(x) for x in rng.choice(nb, size=2, replace=False))
        vals[j1][int(rng.integers(len(rows[j1]))), int(rng.integers(C))] = g
        vals[j2][int(rng.integers(len(rows[j2]))), int(rng.integers(C))] = -g
    if kind not in ("neg_final", "neg_hidden", "ada_tie"):
        for r, v in zip(rows, vals):
            ctx.place_specials(r, v)

    pushes = []
    for b in range(nb):
        buf = encode(cfg, first + rows[b], vals[b])
        if b in cut:
            buf = buf[:cut[b]].copy()
        pushes.append(buf)
    return dict(op="push", kind=kind, pushes=pushes, error=error, error_push=(j if error else None),
                expects=expects, applied=True, bad_row=bad_row, sel=sel)


def _be_bytes(ctx, nrows, raw_ok):
    """Big-endian checkpoint bytes of nrows rows: raw random bits on the plain-sum float
    matrices (no NaN in column 0), generated values elsewhere."""
    rng, cfg = ctx.rng, ctx.cfg
    V = np.dtype(VDT[ctx.vt]).itemsize
    if raw_ok and ctx.vt != I32 and not cfg["ada"] and cfg["data_type"] == MATRIX:
        u = rng.integers(0, 256, size=nrows * ctx.C * V, dtype=np.uint8).view(np.dtype(UDT[ctx.vt]).newbyteorder(">"))
        u = u.reshape(nrows, ctx.C).copy()
        top = 0x40000000 if V == 4 else 0x4000000000000000
        u[:, 0] &= ~np.array(top, u.dtype)  # exponent never all ones
        return u.tobytes()
    if ctx.vt == I32:
        v = rng.integers(1000, 2001, size=(nrows, ctx.C)).astype(np.int32)
    else:
        v = rng.standard_normal((nrows, ctx.C)).astype(VDT[ctx.vt])
    return v.astype(np.dtype(VDT[ctx.vt]).newbyteorder(">")).tobytes()


def _gen_sync(ctx, kind, end, bad_row=None):
    cfg, rng, R = ctx.cfg, ctx.rng, ctx.R
    first, last = cfg["first"], cfg["first"] + R - 1
    op = dict(op="sync", kind=kind, end=end)
    span = max(1, min(R, (1 << 20) // max(_row_bytes(cfg), 1)))  # rows of about 1 MiB at the most
    if kind == "fetch_list":
        n = int(rng.integers(1, 151))
        keys = (first + rng.integers(0, R, size=n)).tolist()
        keys += keys[:int(rng.integers(0, 4))]  # repeats: a KeyList is a set
        outside = [first - 1, last + 1, first - 5000, last + 70_000, first + (1 << 32) + 3, first - (1 << 32) + 3]
        for _ in range(int(rng.integers(1, 4))):
            keys.insert(int(rng.integers(len(keys) + 1)), outside[int(rng.integers(len(outside)))])
        op["keys"] = [int(k) for k in keys]
    elif kind == "fetch_range":
        how = int(rng.integers(3))
        a, b = int(rng.integers(1, 50)), int(rng.integers(0, span))
        if how == 0:
            op["lo"], op["hi"] = first - a, first + b
        elif how == 1:
            op["lo"], op["hi"] = last - b, last + a
        else:
            op["lo"], op["hi"] = first - a, last + a
    elif kind in ("sync_to", "sync_from", "read_rows"):
        if bad_row is not None:
            lo, hi = max(0, bad_row - int(rng.integers(0, 5))), min(R - 1, bad_row + int(rng.integers(0, 5)))
        else:
            lo = int(rng.integers(0, R))
            hi = min(R - 1, lo + int(rng.integers(0, span)))
        op["lo"], op["hi"] = lo, hi
        if kind == "sync_from":
            op["data"] = _be_bytes(ctx, hi - lo + 1, raw_ok=True)
        if kind == "read_rows":
            op["which"] = int(rng.integers(0, 3)) if cfg["ada"] else 0
    elif kind == "read_all":
        op["data"] = _be_bytes(ctx, R, raw_ok=True)
    elif kind == "fill":
        if ctx.vt == I32:
            op["value"] = 1500
        else:
            op["value"] = (0.0, 0.125, -1.5, 0.001)[int(rng.integers(4))]
        # DataStore.set(String) changes the float matrix stores only; elsewhere the fill call itself
        op["as_set"] = bool(cfg["data_type"] == MATRIX and ctx.vt == F32 and rng.random() < 0.5)
    elif kind == "set_alpha":
        op["alpha"] = ((0.05, 0.002, 1.25), (0.025, 0.001, 1.5), (0.1, 0.0005, 2.0))[int(rng.integers(3))]
    return op


def initial_values(cfg, seed):
    rng = np.random.default_rng([zlib.crc32(cfg["name"].encode()), seed, 99])
    shape = (cfg["rows"], cfg["cols"])
    if cfg["value_type"] == I32:
        return rng.integers(1000, 2001, size=shape).astype(np.int32)
    return rng.standard_normal(shape).astype(VDT[cfg["value_type"]])


def plan_bursts(cfg, rng):
    """The call kinds of every burst: every kind of push_kinds(cfg) once where it is applied
    (never behind an error in its burst), fillers up to about 24 ops, at most one error per
    burst and at least a third of the bursts without one. A name ending in "!" is a call
    behind the burst's error: neither side applies it."""
    matrix = cfg["data_type"] == MATRIX
    kinds = push_kinds(cfg)
    errs = [k for k in kinds if k in ERROR_KINDS]
    scripted = ["perm", "ident", "mixed_full", "perm_again"] if matrix else ["arr", "arr_rep", "arr"]
    clean = [k for k in kinds if k not in ERROR_KINDS and k not in scripted]
    fill_from = [k for k in kinds if k not in ERROR_KINDS and k != "long"]
    rng.shuffle(errs)
    rng.shuffle(clean)
    n_clean = max(2, (len(errs) + 1) // 2)           # besides the scripted one
    bursts = [[] for _ in range(n_clean)] + [[k] for k in errs]
    for i, k in enumerate(clean):
        bursts[i % n_clean].append(k)
    n_ops = sum(len(b) for b in bursts) + len(scripted) + len(bursts) + 1
    for _ in range(200):
        if n_ops >= 24:
            break
        b = bursts[int(rng.integers(len(bursts)))]
        if len(b) >= 4:
            continue
        k = fill_from[int(rng.integers(len(fill_from)))]
        err_at = [i for i, name in enumerate(b) if name in ERROR_KINDS]
        if not err_at:
            b.insert(int(rng.integers(len(b) + 1)), k)
        elif rng.random() < 0.5:
            b.insert(int(rng.integers(err_at[0] + 1)), k)   # pipelined in front of the error
        else:
            b.append(k + "!")                                # behind it: dropped or refused
        n_ops += 1
    out = [bursts[i] for i in rng.permutation(len(bursts))]
    out.insert(int(rng.integers(len(out) + 1)), list(scripted))
    return out


def make_sequence(config, seed):
    """[init op, push op.., sync op, push op.., sync op, ...]: see the module docstring."""
    cfg = CONFIGS[config] if isinstance(config, str) else config
    ctx = _Ctx(cfg, seed)
    rng = ctx.rng
    seq = [dict(op="init", values=initial_values(cfg, seed), alpha=ALPHA0 if cfg["ada"] else None)]
    bursts = plan_bursts(cfg, rng)
    deck = sync_kinds(cfg)
    at = (seed % 3) * len(bursts)
    for bi, calls in enumerate(bursts):
        ctx.last_burst = bi == len(bursts) - 1
        errored, bad_row, first_perm = False, None, None
        for name in calls:
            dropped = name.endswith("!")
            kind = name.rstrip("!")
            if kind == "perm_again":
                # the call three chunks after the scripted `perm` one lands in its workspace:
                # the same orders, arriving in another order, take its kept slot columns
                sel = [first_perm["sel"][i] for i in rng.permutation(len(first_perm["sel"]))]
                op = _gen_call(ctx, "perm", sel=sel, nb=len(sel))
                if spec_shaped(cfg):
                    op["expects"].append("reuse")
            elif kind == "perm" and first_perm is None and calls[-1] == "perm_again":
                n = ctx.nb(1, 4) if (cfg["ada"] and flat_shaped(cfg)) else ctx.nb()
                sel = [int(rng.integers(len(ctx.perms))) for _ in range(n)]
                op = first_perm = _gen_call(ctx, "perm", sel=sel, nb=n)
            else:
                op = _gen_call(ctx, kind)
            if dropped or errored:
                op["applied"] = False
            if op["error"] and op["applied"]:
                errored, bad_row = True, op["bad_row"]
            elif op["error"]:
                op["error"] = None  # (fillers are never error kinds; belt and braces)
            seq.append(op)
        kind = "sync_from" if bad_row is not None else deck[(at + bi) % len(deck)]
        seq.append(_gen_sync(ctx, kind, "retire" if bi % 2 == 0 else "drop", bad_row))
    return seq


def bursts_of(seq):
    """[(push ops, sync op), ...] of a sequence."""
    out, cur = [], []
    for op in seq[1:]:
        if op["op"] == "push":
            cur.append(op)
        else:
            out.append((cur, op))
            cur = []
    assert not cur, "a sequence ends with a sync op"
    return out


def expected_paths(seq):
    """Path names the applied calls of a sequence plan to reach (counted from the plan)."""
    out = {}
    for op in seq:
        if op["op"] == "push" and op["applied"] and not op["error"]:
            for e in op["expects"]:
                out[e] = out.get(e, 0) + 1
    return out


def digest(seq):
    h = hashlib.sha256()
    for op in seq:
        h.update(repr(sorted((k, v) for k, v in op.items()
                             if not isinstance(v, (np.ndarray, bytes, list)))).encode())
        if op["op"] == "init":
            h.update(op["values"].tobytes())
        elif op["op"] == "push":
            for p in op["pushes"]:  # (length, CRC-32) per push: sha256 over every byte took half a minute
                h.update(len(p).to_bytes(8, "little"))
                h.update(zlib.crc32(p).to_bytes(4, "little"))
        else:
            h.update(op.get("data", b""))
            h.update(repr(op.get("keys")).encode())
    return h.hexdigest()


# ---- the oracle's side of a sequence -----------------------------------------------------
class OracleSide:
    """Applies ops to a pyoracle.OracleStore and returns what the store under test must show."""

    def __init__(self, pyoracle, cfg, init_op):
        self.cfg = cfg
        self.o = pyoracle.OracleStore(cfg["data_type"], cfg["key_type"], cfg["value_type"], cfg["first"],
                                      cfg["first"] + cfg["rows"] - 1, cfg["cols"], 1, int(cfg["ada"]),
                                      int(cfg["ref_stride"]))
        self.o.data[:] = init_op["values"]
        if cfg["ada"]:
            self.o.set_alpha(*init_op["alpha"])

    def push_call(self, op):
        """Pushes in order until one fails: the (code, key, col) it failed with, or None."""
        for p in op["pushes"]:
            if self.o.push(p.tobytes()):
                return self.o.error()
        return None

    def clear_error(self):
        self.o.clear_error()

    def sync(self, op):
        """Applies a sync op; returns the bytes (or array) the store's call must give, or None."""
        o, cfg, kind = self.o, self.cfg, op["kind"]
        first, last = cfg["first"], cfg["first"] + cfg["rows"] - 1
        be = np.dtype(VDT[cfg["value_type"]]).newbyteorder(">")
        if kind == "fetch_list":
            keys = list(dict.fromkeys(k for k in op["keys"] if first <= k <= last))
            return o.fetch(keys)
        if kind == "fetch_range":
            return o.fetch(np.arange(max(op["lo"], first), min(op["hi"], last) + 1))
        if kind == "write_all":
            return o.write_all()
        if kind == "sync_to":
            return o.data[op["lo"]:op["hi"] + 1].astype(be).tobytes()
        if kind == "sync_from":
            o.data[op["lo"]:op["hi"] + 1] = np.frombuffer(op["data"], be).reshape(-1, cfg["cols"])
        elif kind == "read_all":
            o.data[:] = np.frombuffer(op["data"], be).reshape(o.data.shape)
        elif kind == "fill":
            o.data[:] = op["value"]
        elif kind == "set_alpha":
            o.set_alpha(*op["alpha"])
        elif kind == "read_rows":
            src = o.data if op["which"] == 0 else o.alpha if op["which"] == 1 else o.delta
            return src[op["lo"]:op["hi"] + 1].copy()
        return None

"""Packed push arenas and the case table of tests/test_gpu_geometry.py.

The product places device pushes back to back at 4-byte-aligned addresses (the exchange
path's receive buffer); every other test gives each push its own 256-byte-aligned
allocation followed by allocator slack. `pack` builds the product's layout, with a
poisoned guard band on both sides, so that a read outside a push shows up in the
compared values and a write outside it shows up in the guard check.

Pure numpy: the layout, the poison and the case table are pinned without a GPU by
tests/test_geometry_helper.py; only `Arena.upload` and `OutArena.upload` need torch.
"""
import numpy as np

# One dword that is wrong under every reading the kernels make of push memory:
#   f32: 0x7FF7FFFF is a NaN (exponent 0xFF, mantissa != 0);
#   f64: two of them, 0x7FF7FFFF7FF7FFFF, are a NaN (exponent 0x7FF, mantissa != 0);
#   int32 value: 2 146 959 359; the tests' counters stay below 2^10, so one absorbed
#     poison word moves a sum by 2^31 - 2^19 - 1 (or wraps it negative);
#   key: as int32, as the low word of an int64, and as both words of an int64 it lies
#     outside [first, first + rows) for every first_key the tests use, also after the
#     reference's (int)(key - first) narrowing (poison_row below; pinned per case).
POISON = 0x7FF7FFFF
GUARD = 8192          # bytes of poison before the first and after the last push
GAP = 64              # separated=True: poison bytes between neighbouring pushes
LEADS = (0, 4, 8, 12)  # address of the first push, mod 16


def poison_f32() -> np.float32:
    return np.array([POISON], "<u4").view("<f4")[0]


def poison_f64() -> np.float64:
    return np.array([POISON, POISON], "<u4").view("<f8")[0]


def poison_i32() -> int:
    return int(np.array([POISON], "<u4").view("<i4")[0])


def poison_i64() -> int:
    return int(np.array([POISON, POISON], "<u4").view("<i8")[0])


def row_index(key: int, first: int, rows: int) -> int:
    """The reference's (int)(key - first), -1 outside the shard (oracle row_index)."""
    idx = (key - first) & 0xFFFFFFFF
    if idx >= 1 << 31:
        idx -= 1 << 32
    return idx if 0 <= idx < rows else -1


def poison_row(first: int, rows: int) -> int:
    """Row a key made of poison lands on (-1: outside the shard). Only a key's low
    word enters the narrowed index, so the int32, low-word and both-words readings
    agree; all three are evaluated."""
    got = {row_index(k, first, rows) for k in (poison_i32(), POISON, poison_i64())}
    return -1 if got == {-1} else max(got)


def layout(lens, lead, separated=False):
    """Offsets of the pushes inside the arena and the arena's size in bytes."""
    assert lead in LEADS and all(n >= 0 and n % 4 == 0 for n in lens)
    off, offs = GUARD + lead, []
    for i, n in enumerate(lens):
        if i and separated:
            off += GAP
        offs.append(off)
        off += n
    return offs, off + GUARD + (-off) % 16


class Arena:
    """Input arena: [guard | lead | push 0 | push 1 | ... | guard], poison outside the pushes."""

    def __init__(self, pushes, lead, separated=False):
        pushes = [np.frombuffer(bytes(p), np.uint8) for p in pushes]
        self.lens = [int(p.size) for p in pushes]
        self.offs, total = layout(self.lens, lead, separated)
        self.host = np.full(total // 4, POISON, "<u4").view(np.uint8)
        self.guard = np.ones(total, bool)
        for o, p in zip(self.offs, pushes):
            self.host[o:o + p.size] = p
            self.guard[o:o + p.size] = False
        self.dev = None

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        torch.cuda.synchronize()
        assert self.dev.data_ptr() % 256 == 0  # the offsets alone decide the alignment
        return self

    @property
    def ptrs(self):
        return [self.dev.data_ptr() + o for o in self.offs]

    def check(self):
        """Every guard byte, and every push byte, is as uploaded: no kernel writes push memory."""
        import torch
        torch.cuda.synchronize()
        back = self.dev.cpu().numpy()
        bad = np.flatnonzero(back != self.host)
        assert bad.size == 0, ("arena bytes changed", bad[:8].tolist(), bool(self.guard[bad].any()))


def pack(pushes, lead, separated=False):
    """The device arena of `pushes` (bytes each), first push at arena base + GUARD + lead."""
    return Arena(pushes, lead, separated).upload()


class OutArena:
    """Output placed at base + GUARD + lead inside poison: [guard | lead | nbytes | guard]."""

    def __init__(self, nbytes, lead=0):
        assert lead in LEADS and nbytes % 4 == 0
        self.off, self.nbytes = GUARD + lead, nbytes
        total = self.off + nbytes + GUARD + (-(self.off + nbytes)) % 16
        self.host = np.full(total // 4, POISON, "<u4").view(np.uint8)
        self.dev = None

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        torch.cuda.synchronize()
        assert self.dev.data_ptr() % 256 == 0
        return self

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.off

    def read(self):
        """Copy the arena back and return the output region's bytes."""
        import torch
        torch.cuda.synchronize()
        self.back = self.dev.cpu().numpy()
        return self.back[self.off:self.off + self.nbytes]

    def untouched(self, written):
        """Assert that every byte outside the `written` [(start, stop)) spans of the
        output region (relative to it) still holds poison. Call after read()."""
        keep = np.ones(self.back.size, bool)
        for a, b in written:
            assert 0 <= a <= b <= self.nbytes
            keep[self.off + a:self.off + b] = False
        bad = np.flatnonzero((self.back != self.host) & keep)
        assert bad.size == 0, ("bytes outside the output were written", (bad[:8] - self.off).tolist())


# --------------------------------------------------------------------------- cases
# Fields of a k_reduce_rows instantiation's name, in order (launch_reduce_t's kname).
ROWS_FIELDS = ("type", "MODE", "CPW", "RPW", "NT", "FULL", "DEPTH", "WPB", "SNT")


def kernel_fields(name):
    """'dml::k_x<a, b>' -> ('k_x', ['a', 'b'])."""
    assert name.startswith("dml::"), name
    base, _, rest = name[5:].partition("<")
    return base, ([f.strip() for f in rest.rstrip(">").split(",")] if rest else [])


def kernel_is(name, base, **fields):
    """The launched instantiation is `base`, with the given k_reduce_rows fields
    (others: only `type`, the first template argument). Cases whose kernel has no
    template argument worth pinning (sparse leaves, k_ada_flat, k_ada_ident) pass no
    fields: the base name is what the dispatch decides. Alias cases pass want=None and
    assert no kernel on purpose: their chunk may stay speculative or re-run through
    the key index, and either is correct."""
    b, f = kernel_fields(name)
    assert b == base, (name, base)
    for k, v in fields.items():
        i = ROWS_FIELDS.index(k) if base == "k_reduce_rows" else {"type": 0}[k]
        assert f[i] == str(v), (name, k, v)


BIG33 = (1 << 33) + 7    # first key with a non-zero high word
STRADDLE = (1 << 31) - 50  # the shard's keys straddle 2^31
NEG32 = -1000            # int32 keys: the shard starts below zero
ALIAS = 1 << 32          # added to a key: (int)(key - first) is unchanged


def _c(id, kt, vt, cols, rows, kind, n, want, frac=1.0, first=1000, ada=False, knob=False, calls=1,
       dt=1, alias=False, family=None, **kw):
    return dict(id=id, kt=kt, vt=vt, cols=cols, rows=rows, kind=kind, n=n, want=want, frac=frac, first=first,
                ada=ada, knob=knob, calls=calls, dt=dt, alias=alias, family=family or want[0], **kw)


def _rows(**f):
    return ("k_reduce_rows", f)


MATRIX_CASES = [
    # k_reduce, the generic path: rows narrower than one vector; permuted partial pushes
    _c("generic-c3-f32-i32", 0, 1, 3, 301, "perm", 5, ("k_reduce", dict(type="float")), frac=0.6),
    _c("generic-c1-f64-i64", 1, 3, 1, 301, "perm", 5, ("k_reduce", dict(type="double")), frac=0.6),
    # k_reduce_rows FULL, CPW 4 / 2 / 1 (512 and 256: under half the rows, so use_flat is false)
    _c("full-c1024", 0, 1, 1024, 301, "perm", 3, _rows(type="float", CPW=4, FULL="true", DEPTH=1), frac=0.8),
    _c("full-c512", 0, 1, 512, 301, "perm", 4, _rows(type="float", CPW=2, FULL="true", DEPTH=1), frac=0.45),
    _c("full-c256", 0, 1, 256, 301, "perm", 4, _rows(type="float", CPW=1, FULL="true", DEPTH=1), frac=0.45),
    # k_reduce_rows DEPTH 3, ragged rows (the widths use_flat would take list under half the rows)
    _c("d3-c1000-i32", 0, 0, 1000, 301, "perm", 5, _rows(type="int", CPW=4, FULL="false", DEPTH=3), frac=0.45),
    _c("d3-c700-f32", 0, 1, 700, 301, "perm", 4, _rows(type="float", CPW=2, FULL="false", DEPTH=3), frac=0.45),
    _c("d3-c37-f32", 0, 1, 37, 1237, "perm", 4, _rows(type="float", CPW=1, FULL="false", DEPTH=3), frac=0.45),
    _c("d3-c1500-f32", 0, 1, 1500, 301, "perm", 4, _rows(type="float", CPW=4, FULL="false", DEPTH=3), frac=0.7),
    _c("d3-c510-f64-i64", 1, 3, 510, 301, "perm", 4, _rows(type="double", CPW=4, FULL="false", DEPTH=3), frac=0.45),
    # the same shapes one column off a whole vector (cols % VEC != 0): the last lane's
    # vector is loaded shifted back to end at the row's last element (voff - shb) and the
    # elements selected afterwards; only these widths (and 37 above) take that path
    _c("d3-c1001-i32", 0, 0, 1001, 301, "perm", 5, _rows(type="int", CPW=4, FULL="false", DEPTH=3), frac=0.45),
    _c("d3-c701-f32", 0, 1, 701, 301, "perm", 4, _rows(type="float", CPW=2, FULL="false", DEPTH=3), frac=0.7),
    _c("d3-c1499-f32", 0, 1, 1499, 301, "perm", 4, _rows(type="float", CPW=4, FULL="false", DEPTH=3), frac=0.7),
    _c("d3-c509-f64-i64", 1, 3, 509, 301, "perm", 4, _rows(type="double", CPW=4, FULL="false", DEPTH=3), frac=0.7),
    # k_reduce_flat: dense permuted pushes (one of them not full-range: no speculation)
    _c("flat-c200-f32", 0, 1, 200, 1237, "dense", 4, ("k_reduce_flat", dict(type="float"))),
    _c("flat-c100-f64-i64", 1, 3, 100, 1237, "dense", 4, ("k_reduce_flat", dict(type="double"))),
    # k_flat_ident: ascending full-range pushes; 1, 3 and 9 (the ring of D = 3 pushes wraps)
    *[_c(f"flatident-c200-f32-n{n}", 0, 1, 200, 1237, "asc", n, ("k_flat_ident", dict(type="float")))
      for n in (1, 3, 9)],
    *[_c(f"flatident-c100-f64-i64-n{n}", 1, 3, 100, 1237, "asc", n, ("k_flat_ident", dict(type="double")))
      for n in (1, 3, 9)],
    # speculative chunks of whole 4-KiB rows (k_reduce_rows FULL verifies every key), two calls
    _c("spec-c1024", 0, 1, 1024, 301, "asc", 4, _rows(type="float", CPW=4, FULL="true", DEPTH=1), calls=2, spec=2),
    # 4000-B rows: a flat shape (use_flat) whenever the pushes are full-range, so the
    # ascending chunk runs k_flat_ident at its widest row (1000 of 1024 vector slots);
    # k_reduce_rows' spec_lane needs a speculative chunk that is neither FULL nor flat,
    # which spec_shape never offers
    _c("spec-c1000", 0, 1, 1000, 301, "asc", 4, ("k_flat_ident", dict(type="float")), calls=2, spec=2),
    # k_ada_flat: AdaGrad chunks of <= 4 dense pushes, permuted
    *[_c(f"adaflat-c200-w{w}", 0, 1, 200, 1237, "permfull", w, ("k_ada_flat", {}), ada=True) for w in (1, 4)],
    # k_ada_ident: ascending, every key checked before the launch (threshold lowered)
    *[_c(f"adaident-c{c}-w{w}", 0, 1, c, 1237, "asc", w, ("k_ada_ident", {}), ada=True, knob=True)
      for c in (200, 48) for w in (1, 3)],
    # k_reduce, AdaGrad: more than 4 pushes
    _c("adagen-c200-w6", 0, 1, 200, 301, "permfull", 6, ("k_reduce", dict(type="float")), ada=True,
       family="k_reduce_ada"),
]

# Key geometry: the same shapes with first keys whose high word is set, that straddle
# 2^31, or (int32 keys) below zero; `alias`: a few keys of push 1 are 2^32 too large.
KEY_CASES = [
    *[_c(f"{c['id']}-first{tag}", **{**{k: v for k, v in c.items() if k != "id"}, "first": f})
      for c in MATRIX_CASES if c["kt"] == 1 for tag, f in (("33", BIG33), ("31", STRADDLE))],
    _c("flat-c200-f32-firstneg", 0, 1, 200, 1237, "dense", 4, ("k_reduce_flat", dict(type="float")), first=NEG32),
    _c("flatident-c200-f32-n3-firstneg", 0, 1, 200, 1237, "asc", 3, ("k_flat_ident", dict(type="float")),
       first=NEG32),
    # alias keys: in an ascending set (the chunk may stay speculative or re-run) and in
    # a permuted full-range set (k_reduce_flat's verifying loop)
    *[_c(f"alias-asc-c100-f64-i64-first{tag}", 1, 3, 100, 1237, "asc", 3, None, first=f, alias=True,
         family="alias") for tag, f in (("33", BIG33), ("31", STRADDLE), ("0", 0))],
    *[_c(f"alias-perm-c100-f64-i64-first{tag}", 1, 3, 100, 1237, "permfull", 3, None, first=f, alias=True,
         family="alias") for tag, f in (("33", BIG33), ("31", STRADDLE))],
    _c("alias-asc-c512-f64-i64", 1, 3, 512, 301, "asc", 3, None, first=BIG33, alias=True, family="alias"),
    _c("alias-generic-c1-f64-i64", 1, 3, 1, 301, "perm", 5, None, first=STRADDLE, alias=True, frac=0.6,
       family="alias"),
    # AdaGrad with int64 keys above 2^31: maxDelta's row is the oracle's (int)key
    *[_c(f"adaflat-c200-w4-i64-first{tag}", 1, 1, 200, 1237, "permfull", 4, ("k_ada_flat", {}), ada=True, first=f)
      for tag, f in (("33", BIG33), ("31", STRADDLE))],
    *[_c(f"adaident-c200-w3-i64-first{tag}", 1, 1, 200, 1237, "asc", 3, ("k_ada_ident", {}), ada=True, knob=True,
         first=f) for tag, f in (("33", BIG33), ("31", STRADDLE))],
    _c("adagen-c200-w6-i64-first31", 1, 1, 200, 301, "permfull", 6, ("k_reduce", dict(type="float")), ada=True,
       first=STRADDLE, family="k_reduce_ada"),
]

# Sparse arrays through pushDevice: 8-, 12- and 16-byte records; 50 000-row shard, 4
# pushes of 5 000 keys; push 2 lists a key twice; the int32 array with its check.
SPARSE_CASES = [
    _c("sparse-i32-f32", 0, 1, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=5),
    _c("sparse-i64-f32", 1, 1, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=5),
    _c("sparse-i32-f64", 0, 3, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=5),
    _c("sparse-i64-f64", 1, 3, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=5),
    _c("sparse-i32-i32", 0, 0, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=5),
    _c("sparse-i64-f32-first33", 1, 1, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=BIG33),
    _c("sparse-i64-f64-first31", 1, 3, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=STRADDLE),
    _c("sparse-i64-f32-alias", 1, 1, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=STRADDLE, alias=True),
    _c("sparse-i32-f32-firstneg", 0, 1, 1, 50_000, "sparse", 4, ("k_sp_leaf", {}), dt=0, first=NEG32),
]

ALL_CASES = MATRIX_CASES + KEY_CASES + SPARSE_CASES
ADA = (0.025, 0.0001, 1.5)


def separated_cases():
    """One case per kernel family for the separated=True run: the family's first case
    with at least two pushes (with one push there is no gap, and the arena would equal
    the packed one)."""
    seen, out = set(), []
    for c in ALL_CASES:
        if c["family"] not in seen and c["n"] >= 2:
            seen.add(c["family"])
            out.append(c)
    return out


# Placements of the tests outside the case table (split, pre-reduce, pieces, big leaf):
# (lead, separated); every lead packed, and one separated run.
PLACEMENTS = [(lead, False) for lead in LEADS] + [(4, True)]


def placement_id(p):
    return f"{p[0]}-sep" if p[1] else str(p[0])


def sampled_records(oracle, n):
    """Record positions k_ident_check samples in some push of a chunk (32 evenly spaced
    + 32 hashed per push; tests/test_gpu_parity.py's _sampled_rows, over the first 16 pushes)."""
    out = set()
    for b in range(16):
        out |= {t * (n - 1) // 31 for t in range(32)}
        out |= {oracle.splitmix64((b << 32) + t) % n for t in range(32, 64)}
    return out


def build(case, oracle):
    """(init array, list of push bytes) of a case; deterministic per case id."""
    from distml_amd.store import encode_array_push, encode_matrix_push
    import zlib
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    rows, cols, vt, kt, first = case["rows"], case["cols"], case["vt"], case["kt"], case["first"]
    dt = {0: np.int32, 1: np.float32, 3: np.float64}[vt]
    scale = 0.6 if case["ada"] else 1e-3
    if vt == 0:
        init = rng.integers(100, 200, size=(rows, cols)).astype(np.int32)
    else:
        init = rng.standard_normal((rows, cols)).astype(dt)
    pushes = []
    for b in range(case["n"]):
        kind = case["kind"]
        if kind == "asc":
            r = np.arange(rows)
        elif kind == "permfull":
            r = rng.permutation(rows)
        elif kind == "dense":  # every push lists at least half the rows; push 1 not all of them
            r = rng.permutation(rows)[: rows if b != 1 else (3 * rows) // 4]
        elif kind == "perm":
            r = rng.permutation(rows)[: max(1, int(rows * case["frac"]))]
        else:  # sparse
            r = rng.choice(rows, size=5_000, replace=False)
            if b == 2:
                r[4_000] = r[17]  # one key twice in this push
        keys = first + r.astype(np.int64)
        if case["alias"] and b == min(1, case["n"] - 1):
            free = sorted(set(range(len(r))) - sampled_records(oracle, len(r)))
            for i in (free[3], free[len(free) // 2], free[-2]):
                keys[i] += ALIAS
        if vt == 0:
            v = rng.integers(-2, 3, size=(len(r), cols)).astype(np.int32)
        else:
            v = (rng.standard_normal((len(r), cols)) * scale).astype(dt)
        if case["dt"] == 1:
            pushes.append(encode_matrix_push(keys, v, kt, vt))
        else:
            pushes.append(encode_array_push(keys, v.ravel(), kt, vt))
    return init, pushes


def oracle_run(case, oracle):
    """The sequential oracle on the unpacked pushes: (init, pushes, oracle store, rc of the last push)."""
    init, pushes = build(case, oracle)
    o = oracle.OracleStore(case["dt"], case["kt"], case["vt"], case["first"], case["first"] + case["rows"] - 1,
                           case["cols"], 1, int(case["ada"]), 0)
    if case["ada"]:
        o.set_alpha(*ADA)
    o.data[:] = init
    rc = 0
    for p in pushes:
        rc = o.push(p)
        if rc:
            break
    return init, pushes, o, rc


# ------------------------------------------------------- pre-reduce and group inputs
def prereduce_case(oracle, rows=1000, cols=300, W=5):
    """Five full-range f32 pushes (ascending and four strided orders) and their ordered
    sum from zero: (push bytes, rows x cols f32)."""
    pas = [1, 3, 7, 9, 11]  # coprime with 1000: each push lists every row once
    host = [oracle.synth_dense_bucket(0, 1, 0, rows, rows, cols, 70 + b, pas[b], b).tobytes() for b in range(W)]
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols)
    for h in host:
        assert o.push(h) == 0
    return host, o.data.copy()


def exchange_case(oracle, rows=1237, cols=200):
    """Six AdaGrad key-subset pushes with some keys outside the matrix (the exchange
    path splits them), and the oracle fed the in-matrix records in push order."""
    from distml_amd.store import encode_matrix_push
    rng = np.random.default_rng(91)
    host = []
    for b in range(6):
        keys = rng.permutation(rows + 40)[: rng.integers(100, rows)] - 20
        host.append(encode_matrix_push(keys, (rng.standard_normal((len(keys), cols)) * 0.6).astype(np.float32), 0, 1))
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols, 1, 1)
    o.set_alpha(*ADA)
    for h in host:  # the client's split: out-of-matrix keys never reach the server
        r = np.frombuffer(h, np.uint8).reshape(-1, 4 + 4 * cols)
        k = r[:, :4].copy().view("<i4").ravel()
        assert o.push(r[(k >= 0) & (k < rows)].tobytes()) == 0
    return host, o


def full_range_case(oracle, rows=1000, cols=256, W=5):
    """Five full-range int32 pushes into a synth_fill(3) shard, and the oracle after them."""
    pas = [1, 3, 7, 9, 11]
    host = [oracle.synth_dense_bucket(0, 0, 0, rows, rows, cols, 70 + b, pas[b], 3 * b).tobytes() for b in range(W)]
    o = oracle.OracleStore(1, 0, 0, 0, rows - 1, cols)
    o.synth_fill(3)
    for h in host:
        assert o.push(h) == 0
    return host, o


# The sparse one-level partition (k_sp_leaf_big) on packed records, with pushes that list each key
# once: sparse_plan_big wants >= 8 pushes and a mean of >= kSpBigCap / 6 = 682 records per big
# leaf. With kSpBigBins = 16 384 big leaves that is >= 11.2 M records, and 64 pushes (one chunk)
# then need >= 174 592 distinct keys each, so > 8 x 16 384 rows: 262 144 rows (big leaves of 16
# rows), 64 x 180 000 keys. This is not the smallest such shard: the route model
# (tests/sparse_route.py) finds 131 073 rows, still big leaves of 16 rows but only 8 193 of them,
# so 5.59 M records; tests/sparse_cases.py's big cases use 8 193 big leaves too. The shape stays
# as it is: it is the one with every big leaf the histogram can hold.
BIG_LEAF = dict(first=5, rows=262_144, n=64, per=180_000)


def big_leaf_case(oracle):
    from distml_amd.store import encode_array_push
    c = BIG_LEAF
    rng = np.random.default_rng(2262)
    init = rng.standard_normal((c["rows"], 1)).astype(np.float32)
    o = oracle.OracleStore(0, 1, 1, c["first"], c["first"] + c["rows"] - 1)
    o.data[:] = init
    host = []
    for b in range(c["n"]):
        keys = c["first"] + rng.choice(c["rows"], size=c["per"], replace=False)
        host.append(encode_array_push(keys, (rng.standard_normal(c["per"]) * 1e-2).astype(np.float32), 1, 1))
        assert o.push(host[-1]) == 0
    return init, host, o


# ------------------------------------------------------------------------------ split
SPLIT_CASES = [
    # (data_type, key_type, value_type, cols, total_rows, world, n, nrec): the first five
    # tuples of test_gpu_parity.test_shard_split_kernel, and its first `asc` one
    (1, 0, 1, 200, 5000, 8, 3, 4000),
    (1, 0, 0, 1000, 1000, 3, 2, 700),
    (1, 1, 3, 10, 784, 2, 4, 300),
    (0, 1, 1, 1, 10**9, 5, 2, 20000),
    (1, 0, 1, 64, 100, 64, 1, 257),
    (1, 0, 1, 200, 5003, 8, 3, 5003, "asc"),
]


def np_split(recs_list, K, total_rows, world):
    """Reference split for dml_shard_split: stable per-owner partition, dest-major;
    keys compared as 64-bit values."""
    from distml_amd.datadesc import KeyRange
    step = KeyRange(0, total_rows - 1).linearSplit(world)[0].size()
    kdt = "<i4" if K == 4 else "<i8"
    owners = []
    for r in recs_list:
        k = r[:, :K].copy().view(kdt).ravel().astype(np.int64)
        o = np.where((k >= 0) & (k < total_rows), k // max(step, 1), world)
        owners.append(np.minimum(o, world))
    out = b"".join(r[o == d].tobytes() for d in range(world) for r, o in zip(recs_list, owners))
    counts = [[int((o == d).sum()) for d in range(world)] for o in owners]
    return out, counts


def split_case(case):
    """The record arrays of a SPLIT_CASES tuple: random bytes with keys in
    [-3, total + 3) (`asc`: ascending, push b starting b below zero); int64 keys also
    hold total_rows + 2^32, 5 + 2^32 and -2^32 + 5, which a 64-bit compare drops."""
    dtp, kt, vt, cols, total, world, n, nrec = case[:8]
    asc = len(case) > 8
    K, V = (4 if kt == 0 else 8), (4 if vt in (0, 1) else 8)
    stride = K + (V * cols if dtp == 1 else V)
    rng = np.random.default_rng(sum(case[:8]))
    recs = []
    for b in range(n):
        r = rng.integers(0, 256, size=(nrec + b, stride), dtype=np.uint8)
        keys = rng.integers(-3, total + 3, size=nrec + b).astype("<i4" if K == 4 else "<i8")
        if asc:
            keys = (np.arange(nrec + b) - b).astype(keys.dtype)  # push b: one key below 0 (dropped)
        if K == 8:
            keys[7 + b] = total + (1 << 32)       # low word total: out of the matrix either way
            keys[11 + b] = 5 + (1 << 32)          # low word 5: an in-matrix key's alias
            keys[nrec // 2 + b] = -(1 << 32) + 5  # the same, from below
        r[:, :K] = keys.view(np.uint8).reshape(-1, K)
        recs.append(r)
    return recs, K


def split_owner(key, total_rows):
    """In the matrix or not, as dml_shard_split decides it: the whole 64-bit key."""
    return 0 <= key < total_rows

"""The case table of tests/test_gpu_sparse_edges.py: array chunks built at the smallest shape
that puts a record count exactly on, and one past, each capacity comparison of the sparse
path (dml_sparse.hip), and on each branch of sparse_replay. Pure numpy, so that
tests/test_sparse_route.py can check without a GPU that every case is on the route it
declares (tests/sparse_route.py is the model) and that the order-sensitive ones tell orders
of adds apart.

A case declares, per chunk of <= 64 pushes, what sparse_route.route must return for its keys:
  big, compact   the plan's two layout decisions at launch
  counted        which capacities overflowed (cap1 / cap2 / capS), or compact_cut
  flagged        why leaves were flagged: records / bucket / row_twice_in_push
  branch         sparse_replay's branch (1-4) or None
`pair` names the other member of a boundary pair and `flips` the one predicate
(sparse_route.predicates) in which the two differ. `err`: the error the chunk plans (key = a
key outside the shard, neg = an int32 counter left negative, trunc = a push that ends inside a
record); the GPU test compares code and key with the oracle's. 
`order`: rows whose adds arrive in an order that matters; `swap`: two records of one push on one row.

Values: floats are N(0, 1) x 2^k, k in [-30, 10), so that every order of a row's adds rounds
differently; about 3 % of the records outside the `order` rows carry a special value chosen by
the row's class (row % 7: 0 -> +Inf or the largest finite, 1 -> -Inf or the most negative
finite, 2 -> +-0.0 or a denormal), which keeps +Inf and -Inf on different rows: no NaN arises
(x86's and the GPU's default NaN differ in sign, which is not what these cases are about).
int32 values are small and the counters start high, so only a planned record goes negative.
"""
import zlib

import numpy as np

import sparse_route as R

BIG33 = (1 << 33) + 7   # geom.BIG33: first key with a non-zero high word (int64 keys)
NEG32 = -1000           # geom.NEG32: the shard starts below zero (int32 keys)
TAG = {R.F32: "f32", R.F64: "f64", R.I32: "i32"}
DT = {R.F32: np.dtype("<f4"), R.F64: np.dtype("<f8"), R.I32: np.dtype("<i4")}
OUT = -1                # a record whose key lies outside the shard (first + rows + 5)
NEG_VALUE = -100_000    # the planned int32 add that leaves a counter negative

CASES = []


def _claim(big=False, compact=None, counted=(), flagged=(), branch=None):
    return dict(big=big, compact=compact, counted=tuple(counted), flagged=tuple(flagged), branch=branch)


def _add(id, vt, rows, build, claims, first=5, kt=1, err=None, order=(), pair=None, flips=None, check=None,
         heavy=False):
    if isinstance(claims, dict):
        claims = [claims]
    for c in claims:
        if c["compact"] is None:
            c["compact"] = vt == R.F32
    CASES.append(dict(id=f"{id}-{TAG[vt]}", vt=vt, kt=kt, first=first, rows=rows, build=build, claims=claims,
                      err=err, order=tuple(order), pair=f"{pair}-{TAG[vt]}" if pair else None, flips=flips,
                      check=check, heavy=heavy))


def _pick(rng, lo, hi, n, avoid=()):
    """n distinct rows of [lo, hi) outside `avoid`."""
    pool = np.setdiff1d(np.arange(lo, hi), np.asarray(list(avoid), np.int64)) if len(avoid) else np.arange(lo, hi)
    return rng.choice(pool, size=n, replace=False)


def _spread(total, nb):
    """total split over nb pushes, the remainder on the last ones."""
    return [total // nb + (1 if b >= nb - total % nb else 0) for b in range(nb)]


def apis(case):
    """The entries a case runs through: handlePushBatch and pushDevice both where the chunk leaves
    the plain single pass (counted, or a replay), else one of them, chosen by the id's checksum."""
    if any(c["counted"] or c["branch"] for c in case["claims"]):
        return ("batch", "device")
    return (("batch", "device")[zlib.crc32(case["id"].encode()) % 2],)


# ---- builders: rng -> dict(rows=[row indices per push], neg=[(push, record)]) -----------------
def hot_region(rows, nb, per, hot_hi, n_hot, always=()):
    """nb pushes of `per` distinct rows each; rows [0, hot_hi) receive n_hot records in all, the
    rows `always` (inside it) one from every push."""
    def build(rng):
        out = []
        for h in _spread(n_hot, nb):
            r = np.concatenate([np.asarray(always, np.int64), _pick(rng, 0, hot_hi, h - len(always), avoid=always),
                                _pick(rng, hot_hi, rows, per - h)])
            out.append(rng.permutation(r))
        return dict(rows=out)
    return build


BKT = dict(rows=65536, nb=64, per=128, hot=12345, ordinary=40000)  # SL 13: leaves of 8 192 rows, 8-row buckets


def bucket(kind, n, cut=None, neg=(), trunc=None, neighbour=False):
    """64 pushes of 128 records into 65 536 rows. Record 7 of every push lies in the line bucket of
    row 12 345 (rows 12 344..12 351): `one_row` on that row, `spread` on row 12 344 + push % 8. n = 65:
    record 9 of push 10 is one more (the same row again, or with `neighbour` row 12 346 / another row
    of the bucket); `one_row` without `neighbour` names the two same-push records as `swap`. Record 20 of
    pushes 5 and 40 is row 40 000, in an ordinary leaf. cut: the (push, record) that becomes a key outside the
    shard; neg: (push, "hot" | "ordinary") records that carry NEG_VALUE; trunc: the push that ends
    inside a record (4 bytes of one more)."""
    c = BKT
    b0 = c["hot"] & ~7

    def build(rng):
        out = []
        for b in range(c["nb"]):
            r = _pick(rng, 0, c["rows"], c["per"], avoid=list(range(b0, b0 + 8)) + [c["ordinary"]])
            r[7] = c["hot"] if kind == "one_row" else b0 + b % 8
            if b in (5, 40):
                r[20] = c["ordinary"]
            if n == 65 and b == 10:
                r[9] = (c["hot"] + neighbour) if kind == "one_row" else b0 + (b + 3) % 8
            if cut and cut[0] == b:
                r[cut[1]] = OUT
            out.append(r)
        return dict(rows=out, neg=[(b, 7 if w == "hot" else 20) for b, w in neg], trunc=trunc,
                    swap=(10, 7, 9) if n == 65 and kind == "one_row" and not neighbour else None)
    return build


def few(rows, nb, per, always=(), twice=None, cut=None, neg=()):
    """nb pushes of `per` distinct random rows, each listing the rows `always` at records 0..;
    twice = (push, i, j): record i repeats record j's row (the two are the case's `swap`);
    cut / neg: (push, record)."""
    def build(rng):
        out = []
        for b in range(nb):
            r = _pick(rng, 0, rows, per - len(always), avoid=always)
            r = np.concatenate([np.asarray(always, np.int64), r])
            if twice and twice[0] == b:
                r[twice[1]] = r[twice[2]]
            if cut and cut[0] == b:
                r[cut[1]] = OUT
            out.append(r)
        return dict(rows=out, neg=list(neg), swap=(twice[0], twice[2], twice[1]) if twice else None)
    return build


def every_row(rows, nb):
    """nb pushes, each a permutation of every row of the shard."""
    return lambda rng: dict(rows=[rng.permutation(rows) for _ in range(nb)])


LEAF_ORD = (3, 500, 1023)
# ---- leaf capacity: cap2 == kSpLeafCap. 8 192 rows, 4 x 2 048 records: SL 10, 8 leaves, mean 1 024
for vt in (R.F32, R.F64, R.I32):
    # (cap2 == kSpLeafCap here, so one record more flips two predicates at once: the partition's
    # overflow and the leaf's own limit; rows 3, 500 and 1 023 of the full leaf are in every push)
    _add("leafcap-2048", vt, 8192, hot_region(8192, 4, 2048, 1024, 2048, always=LEAF_ORD), _claim(),
         pair="leafcap-2049", flips=("cap2", "leaf_records"), order=LEAF_ORD)
    _add("leafcap-2049", vt, 8192, hot_region(8192, 4, 2048, 1024, 2049, always=LEAF_ORD),
         _claim(counted=["cap2"], flagged=["records"], branch=4), order=LEAF_ORD)
# ---- cap2 below the leaf capacity: 4 x 1 500 records, mean 750, cap2 = 2 * 750 + 256 = 1 756
for vt in (R.F32, R.F64):
    _add("cap2-1756", vt, 8192, hot_region(8192, 4, 1500, 1024, 1756), _claim(), pair="cap2-1757", flips=("cap2",),
         check=lambda p: p["cap2"] == 1756)
    _add("cap2-1757", vt, 8192, hot_region(8192, 4, 1500, 1024, 1757), _claim(counted=["cap2"]))
# ---- cap1 alone: 24 576 rows, 64 x 6 250 records: SL 5, 768 leaves, 3 level-1 bins of 8 192 rows,
# cap1 = 2 * (400 000 / 3) + 4 096 = 270 762 against 256 leaves x cap2 (1 296) = 331 776
CAP1 = 2 * (400_000 // 3) + 4096
for vt in (R.F32, R.F64):
    _add("cap1-full", vt, 24576, hot_region(24576, 64, 6250, 8192, CAP1), _claim(), pair="cap1-over",
         flips=("cap1",), check=lambda p: p["cap1"] == CAP1 and p["nbins1"] == 3 and p["cap2"] == 1296)
    _add("cap1-over", vt, 24576, hot_region(24576, 64, 6250, 8192, CAP1 + 1), _claim(counted=["cap1"]))
# ---- line bucket: 64 against 65 applied records in one bucket (kSpBucketMax)
ORD_B = tuple(range(BKT["hot"] & ~7, (BKT["hot"] & ~7) + 8))
for vt in (R.F32, R.F64, R.I32):
    replay = 2 if vt == R.F32 else 3
    # all on one row, one per push: the longest leaf_chain; compact words reach push index 63
    # (64 records is all one row takes from a chunk of compact words, so the 65th of the fp32
    # member lies on the next row of the same bucket; f64 and i32 list the row twice in push 10)
    _add("bucket-onerow-64", vt, BKT["rows"], bucket("one_row", 64), _claim(), order=[BKT["hot"]],
         pair="bucket-onerow-65", flips=("bucket",), check=lambda p: p["bshift"] == 3 and p["cap2"] == 2048)
    _add("bucket-onerow-65", vt, BKT["rows"], bucket("one_row", 65, neighbour=vt == R.F32),
         _claim(flagged=["bucket"], branch=replay), order=[BKT["hot"]])
    _add("bucket-spread-64", vt, BKT["rows"], bucket("spread", 64), _claim(), order=ORD_B,
         pair="bucket-spread-65", flips=("bucket",))
    _add("bucket-spread-65", vt, BKT["rows"], bucket("spread", 65), _claim(flagged=["bucket"], branch=replay),
         order=ORD_B)
# int32: a negative counter inside the replayed leaf, and one in an ordinary leaf; the earlier wins
_add("bucket-neg-replayed-first", R.I32, BKT["rows"], bucket("one_row", 65, neg=[(5, "hot"), (40, "ordinary")]),
     _claim(flagged=["bucket"], branch=3), err="neg")
_add("bucket-neg-ordinary-first", R.I32, BKT["rows"], bucket("one_row", 65, neg=[(5, "ordinary"), (40, "hot")]),
     _claim(flagged=["bucket"], branch=3), err="neg")
# a bucket of 65 with a sequence cut through it: replay branch 3 under a cut
for vt in (R.F64, R.I32):
    _add("bucket-spread-65-cut", vt, BKT["rows"], bucket("spread", 65, cut=(40, 3)),
         _claim(flagged=["bucket"], branch=3), err="key", order=ORD_B if vt == R.F64 else ())
# fp32 full records through the single pass: a ragged tail switches compact words off, and the
# flagged leaf then takes branch 3 for fp32 too (every record is applied: the tail is the last push's)
_add("bucket-spread-65-trunc", R.F32, BKT["rows"], bucket("spread", 65, trunc=63),
     _claim(compact=False, flagged=["bucket"], branch=3), err="trunc", order=ORD_B)
# ---- compact words
_add("compact-26", R.F32, 1 << 20, few(1 << 20, 1, 16), _claim(compact=True), pair="compact-27",
     flips=("compact_at_launch",), check=lambda p: p["SL"] + p["D2"] == 26)
_add("compact-27", R.F32, 1 << 20, few(1 << 20, 1, 8), _claim(compact=False), check=lambda p: p["SL"] + p["D2"] == 27)
# 65 pushes: a chunk of 64 and a chunk of one; row 777 in every push
_add("compact-65-pushes", R.F32, 4096, few(4096, 65, 100, always=[777]), [_claim(), _claim()], order=[777])
# push 2 lists row 31 twice (records 0 and 4 000): compact words cannot order the two (branch 2);
# the same keys as f64 can
_add("row-twice", R.F32, 50_000, few(50_000, 4, 5000, always=[31], twice=(2, 4000, 0)),
     _claim(flagged=["row_twice_in_push"], branch=2), order=[31])
_add("row-twice", R.F64, 50_000, few(50_000, 4, 5000, always=[31], twice=(2, 4000, 0)), _claim(), order=[31])
# the last row of level-1 bin 0 and the first of bin 1: 10 240 rows, 20 x 10 000 records, SL 5, 320 leaves
_add("bin-edge", R.F32, 10_240, few(10_240, 20, 10_000, always=[8191, 8192]), _claim(), order=[8191, 8192],
     check=lambda p: p["nbins1"] == 2 and (8191 >> p["SL"]) >> p["D2"] == 0 and (8192 >> p["SL"]) >> p["D2"] == 1)
# ---- cutoff: a key outside the shard; 3 pushes of 6 000 records into 50 000 rows
for vt in (R.F64, R.I32, R.F32):
    for tag, pos in (("first", (0, 0)), ("last", (2, 5999)), ("4095", (1, 4095)), ("4096", (1, 4096))):
        _add(f"cut-{tag}", vt, 50_000, few(50_000, 3, 6000, cut=pos),
             _claim(counted=["compact_cut"] if vt == R.F32 else []), err="key")
# int32: a cutoff and a negative counter, in either order
_add("cut-after-neg", R.I32, 50_000, few(50_000, 3, 6000, cut=(1, 4095), neg=[(0, 100)]), _claim(), err="neg")
_add("cut-before-neg", R.I32, 50_000, few(50_000, 3, 6000, cut=(1, 10), neg=[(2, 50)]), _claim(), err="key")
# ---- shard edges
for vt in (R.F32, R.F64, R.I32):
    _add("rows-1", vt, 1, every_row(1, 9), _claim(), order=[0] if vt != R.I32 else [])
for rows in (31, 33):
    _add(f"rows-{rows}", R.F32, rows, every_row(rows, 6), _claim(), order=[0, rows - 1], kt=0, first=NEG32)
for rows in (15, 17):
    _add(f"rows-{rows}", R.F64, rows, every_row(rows, 6), _claim(), order=[0, rows - 1], first=BIG33)
# a last leaf of one row: 8 * 2^10 + 1 rows; keys first and first + rows - 1 in every push
_add("last-leaf-one-row", R.F32, 8193, few(8193, 4, 2048, always=[0, 8192]), _claim(), order=[0, 8192], kt=0,
     first=NEG32, check=lambda p: p["SL"] == 10 and p["nleaves"] == 9)
_add("last-leaf-one-row", R.F64, 8193, few(8193, 4, 2048, always=[0, 8192]), _claim(), order=[0, 8192],
     first=BIG33, check=lambda p: p["SL"] == 10 and p["nleaves"] == 9)


# ---- big leaves (the one-level partition): fp32, >= 8 pushes, a mean of >= kSpBigCap / 6 = 682 records
# per big leaf. A row takes one record per push (compact words), so 682 records need big leaves of
# >= 16 rows (BL 4) at 64 pushes: > 8 x 16 384 rows, and then nbig = 8 193, >= 5.59 M records. A big
# leaf of kSpBigCap = 4 096 records and one more needs > 64 rows at 64 pushes, and 8 pushes need
# 682 / 8 > 64 rows: BL 7, 8 193 x 128 rows, 64 x 87 320 or 8 x 698 560 records; capS = 2 * 85 + 512.
BIG = dict(rows=8193 * 128, hot=4000, n64=87_320, n8=698_560)
BIG_N = 64 * BIG["n64"]
assert BIG_N == 8 * BIG["n8"]


def big(nrecs, hot):
    """Push b: nrecs[b] distinct rows, hot[b] of them in big leaf 4 000 (rows 512 000..512 127)."""
    lo = BIG["hot"] * 128

    def build(rng):
        out = []
        for n, h in zip(nrecs, hot):
            r = rng.choice(BIG["rows"] - 128, size=n - h, replace=False)
            r[r >= lo] += 128
            out.append(rng.permutation(np.concatenate([lo + rng.choice(128, size=h, replace=False), r])))
        return dict(rows=out)
    return build


def _big_plan(BL=7, capS=682):
    return lambda p: (p["BL"], p["SL"], p["nbig"], p["capS"], p["bshift"]) == (BL, 7, 8193, capS, 0)


_HOT_ORDER = [BIG["hot"] * 128 + i for i in range(4)]
_add("big-4096", R.F32, BIG["rows"], big([BIG["n64"]] * 64, [64] * 64), _claim(big=True), kt=0, heavy=True,
     pair="big-4097", flips=("leaf_records",), check=_big_plan(), order=_HOT_ORDER)
_add("big-4097", R.F32, BIG["rows"], big([BIG["n64"]] * 64, [64] * 63 + [65]),
     _claim(big=True, flagged=["records"], branch=1), kt=0, heavy=True, order=_HOT_ORDER)
# one (big leaf, slice) region: slice 0 = pushes 0, 8, .., 56; the big leaf stays under kSpLeafCap, so
# the counted partition's leaf (SL = BL) is applied without a replay
_S0 = {0: 85, 8: 85, 16: 85, 24: 85, 32: 85, 40: 85, 48: 86, 56: 86}
_add("big-capS-full", R.F32, BIG["rows"], big([BIG["n64"]] * 64, [_S0.get(b, 20) for b in range(64)]),
     _claim(big=True), kt=0, heavy=True, pair="big-capS-over", flips=("capS",), check=_big_plan())
_add("big-capS-over", R.F32, BIG["rows"], big([BIG["n64"]] * 64, [_S0.get(b, 20) + (b == 56) for b in range(64)]),
     _claim(big=True, counted=["capS"]), kt=0, heavy=True)
# 7 pushes against 8 (kSpSlices)
_add("big-8-pushes", R.F32, BIG["rows"], big([BIG["n8"]] * 8, [8] * 8), _claim(big=True), kt=0, heavy=True,
     pair="big-7-pushes", flips=("big",), check=_big_plan())
_add("big-7-pushes", R.F32, BIG["rows"], big(_spread(BIG_N, 7), [8] * 7), _claim(), kt=0, heavy=True)
# slice shares: the largest slice at exactly 5/4 of the mean, and one record past it
_X = (BIG_N * 5 // 4) // 8
_add("big-share-in", R.F32, BIG["rows"], big([_X] + _spread(BIG_N - _X, 7), [8] * 8), _claim(big=True), kt=0,
     heavy=True, pair="big-share-out", flips=("big",), check=_big_plan(capS=2 * (_X // 8193) + 512))
_add("big-share-out", R.F32, BIG["rows"], big([_X + 1] + _spread(BIG_N - _X - 1, 7), [8] * 8), _claim(), kt=0,
     heavy=True)

REQUIRED_F32_BRANCHES = (1, 2, 3, 4)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
_BUILT = {}
_ROUTES = {}


def built(case):
    """dict(keys=[int64 keys per push], vals=[values per push], init=[rows, 1]); once per case."""
    if case["id"] in _BUILT:
        return _BUILT[case["id"]]
    if case["heavy"]:  # tens of MB each: only the latest stays
        for k in [k for k in _BUILT if BY_ID[k]["heavy"]]:
            del _BUILT[k]
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    vt, rows, first = case["vt"], case["rows"], case["first"]
    b = case["build"](rng)
    keys, vals = [], []
    for r in b["rows"]:
        r = np.asarray(r, np.int64)
        keys.append(first + np.where(r == OUT, rows + 5, r))
        if vt == R.I32:
            v = rng.integers(-2, 3, size=len(r)).astype(np.int32)
        else:
            v = (rng.standard_normal(len(r)) * np.float64(2.0) ** rng.integers(-30, 10, size=len(r))).astype(DT[vt])
            fi = np.finfo(DT[vt])
            special = {0: [np.inf, fi.max], 1: [-np.inf, fi.min], 2: [0.0, -0.0, fi.smallest_subnormal,
                                                                      -fi.smallest_subnormal * 3]}
            pick = (rng.random(len(r)) < 0.03) & ~np.isin(r, case["order"]) & (r >= 0)
            for cls, sv in special.items():
                m = pick & (r % 7 == cls)
                v[m] = np.asarray(sv, DT[vt])[rng.integers(len(sv), size=int(m.sum()))]
        vals.append(v)
    for p, i in b.get("neg", []):
        vals[p][i] = NEG_VALUE
    if vt == R.I32:
        init = rng.integers(1000, 2000, size=(rows, 1)).astype(np.int32)
    else:
        init = rng.standard_normal((rows, 1)).astype(DT[vt])
    swap = b.get("swap")
    if vt != R.I32 and case["order"]:
        _separate(rng, b["rows"], vals, init, case["order"], swap, DT[vt])
    # a following small, ordinary chunk on the same store (the workspace under another layout)
    n2 = min(rows, 200)
    k2 = [first + rng.choice(rows, size=n2, replace=False) for _ in range(2)]
    v2 = [rng.integers(0, 3, size=n2).astype(np.int32) if vt == R.I32
          else rng.standard_normal(n2).astype(DT[vt]) for _ in range(2)]
    _BUILT[case["id"]] = dict(keys=keys, vals=vals, init=init, keys2=k2, vals2=v2, trunc=b.get("trunc"),
                              swap=swap)
    return _BUILT[case["id"]]


def _separate(rng, rows, vals, init, order, swap, dt):
    """Values for the records of the `order` rows such that each row's final bits change when its
    applied records are added in reversed order, and, where `swap` = (push, i, j) names two records
    of one push on one row, also when just those two change places. A row of fewer than 32 records
    draws like magnitudes (each add rounds), a longer chain the wide spread of exponents; a draw
    is kept when a plain sequential sum in dt says the orders differ.
    (tests/test_sparse_route.py checks the effect with the oracle, not with this sum.)"""
    stop = next(((b, int(np.flatnonzero(np.asarray(r) == OUT)[0])) for b, r in enumerate(rows)
                 if (np.asarray(r) == OUT).any()), (len(rows), 0))  # the cutoff: nothing from here on is applied

    def total(row, seq):
        x = dt.type(init[row, 0])
        for b, k in seq:
            x = dt.type(x + vals[b][k])
        return x
    for row in order:
        seq = [(b, int(k)) for b, r in enumerate(rows) for k in np.flatnonzero(np.asarray(r) == row)
               if (b, int(k)) < stop]
        alts = [seq[::-1]]
        if swap and rows[swap[0]][swap[1]] == row:
            p, i, j = swap
            assert rows[p][j] == row and i < j and (p, j) < stop
            alts.append([(p, j) if e == (p, i) else (p, i) if e == (p, j) else e for e in seq])
        lo, hi = (-2, 2) if len(seq) < 32 else (-30, 10)
        for _ in range(500):
            a = total(row, seq)
            if np.isfinite(a) and all(a.tobytes() != total(row, alt).tobytes() for alt in alts):
                break
            for (b, k), v in zip(seq, rng.standard_normal(len(seq)) * 2.0 ** rng.integers(lo, hi, size=len(seq))):
                vals[b][k] = v
        else:
            raise AssertionError(("no order-separating values found", row))


def chunks(seq):
    """A batch's pushes in chunks of kMaxW (run_batch, dml_store.hip:576-644)."""
    return [seq[i:i + R.K_MAX_W] for i in range(0, len(seq), R.K_MAX_W)]


def routes(case):
    """sparse_route.route of each chunk of the case's pushes."""
    if case["id"] in _ROUTES:
        return _ROUTES[case["id"]]
    b = built(case)
    assert b["trunc"] is None or len(b["keys"]) <= R.K_MAX_W
    _ROUTES[case["id"]] = [R.route(case["vt"], case["first"], case["rows"], ks, tail=b["trunc"]) for ks in chunks(b["keys"])]
    return _ROUTES[case["id"]]


def encode(case, keys, vals, trunc=None):
    from distml_amd.store import encode_array_push
    out = [encode_array_push(np.ascontiguousarray(k), np.ascontiguousarray(v), case["kt"], case["vt"])
           for k, v in zip(keys, vals)]
    if trunc is not None:
        out[trunc] += b"\x01" * 4  # the start of one more record (device pushes are whole dwords): a truncated access
    return out


def oracle_store(oracle, case):
    return oracle.OracleStore(0, case["kt"], case["vt"], case["first"], case["first"] + case["rows"] - 1)

"""The yardstick of the two-moment AdaGrad kernels (dml_prereduce_moments_piece ->
k_moments_flat; dml_store_apply_adagrad_moments_device -> k_ada_moments + k_maxdelta_elems),
beside tests/chain_ada_expect.py: what their outputs must hold, byte for byte. Plain numpy
on float32 arrays; every float32 operation below rounds once, as the kernels' __fadd_rn /
__fmul_rn do. Written from include/distml_ps.h and the reference's update
(FloatMatrixStoreAdaGrad.java:262-277), never from what a kernel prints.

piece_expect   task row t is model row (t // row_block) * row_stride + row_off + t % row_block;
               its Σu starts at +0.0 and takes the gradient of every push that lists the row,
               in push order; Σu² takes f32(u * u) the same way. Rows at or beyond `rows`, rows
               no push lists, and every row of a call whose index fails (a key outside the
               matrix, a row listed twice in one push) are +0.0 in both halves.
apply_expect   data + Σu, nd = delta + Σu²; alpha = f(nd) where nd > 1 (the store's double
               formula, clamped up to minAlpha), kept elsewhere (NaN included; Inf gives
               minAlpha); maxDelta: the candidates are the elements with nd > delta, the best
               one has the largest nd, then the lowest row-major index, and replaces the
               running record only when strictly above it.

The rest of the module are the inputs of tests/test_gpu_moments.py, generated without a GPU so
that tests/test_moments_expect.py can check on the CPU that they are what they claim to be.
"""
import numpy as np

VT = 1  # FloatMatrixStoreAdaGrad: fp32 values, int keys
F32 = np.dtype("<f4")
NAN_BITS = 0x7FC12345  # tests/opseq.py's payload
ADA = (0.025, 0.0001, 1.5)  # initialAlpha, minAlpha, factor
K_MOMENT_BLOCKS = 2048  # kMomentBlocks (dml_internal.h): k_ada_moments' grid, 256 threads each
IDENT_MIN_BYTES = 64 << 20  # kIdentFullMinBytes (dml_host.h)


def slot_stride(nb):
    """dml_internal.h: a call's slot-table row stride, its push count rounded up to 8."""
    return (nb + 7) & ~7


def rows_per_wave(cols):
    """launch_moments: R = min(16, 512 / (cols / 4)) task rows per wave."""
    return max(1, min(16, 512 // (cols // 4)))


# ---- record codec ------------------------------------------------------------------------
def encode(keys, vals):
    from distml_amd.store import encode_matrix_push
    return np.frombuffer(encode_matrix_push(keys, vals, 0, VT), np.uint8).copy()


def decode(push, cols):
    """(keys int64, gradients [n, cols] f32) of one push."""
    rec = np.frombuffer(bytes(push), np.uint8).reshape(-1, 4 + 4 * cols)
    return rec[:, :4].copy().view("<i4").ravel().astype(np.int64), rec[:, 4:].copy().view(F32)


# ---- the model ---------------------------------------------------------------------------
def sums(pushes, rows, cols, first=0):
    """(Σu, Σu², ok) over the whole matrix; ok False: the call's index fails."""
    su = np.zeros((rows, cols), F32)
    s2 = np.zeros((rows, cols), F32)
    ok = True
    for p in pushes:
        keys, g = decode(p, cols)
        r = keys - first
        if ((r < 0) | (r >= rows)).any() or len(np.unique(r)) != len(r):
            ok = False
            continue
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            su[r] = su[r] + g              # distinct rows: one rounding per add, push order
            s2[r] = s2[r] + (g * g)        # f32(u * u), then the add
    return su, s2, ok


def piece_expect(pushes, rows, cols, row_block, row_stride, row_off, ntask, first=0):
    """[ntask, 2 * cols] f32: what dml_prereduce_moments_piece writes at dev_out."""
    out = np.zeros((ntask, 2 * cols), F32)
    su, s2, ok = sums(pushes, rows, cols, first)
    if not ok:
        return out
    t = np.arange(ntask)
    m = (t // row_block) * row_stride + row_off + t % row_block
    inside = m < rows
    out[inside, :cols] = su[m[inside]]
    out[inside, cols:] = s2[m[inside]]
    return out


def alpha_of(nd, ada):
    """(float)(initialAlpha / (factor * sqrt((double) nd))), clamped up to minAlpha; the
    parameters as the floats a store holds."""
    ia, mn, fa = (np.float32(x) for x in ada)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (np.float64(ia) / (np.float64(fa) * np.sqrt(nd.astype(np.float64)))).astype(F32)
    return np.where(a < mn, mn, a).astype(F32)


def apply_expect(data, delta, alpha, md, src, ada, first):
    """The new (data, delta, alpha, md) after one dml_store_apply_adagrad_moments_device of
    `src` ([rows, 2 * cols] f32); md = (value, row, col), row a key."""
    rows, cols = data.shape
    su, s2 = src[:, :cols], src[:, cols:]
    with np.errstate(over="ignore", invalid="ignore"):
        ndata = (data + su).astype(F32)
        nd = (delta + s2).astype(F32)
    above = nd > np.float32(1.0)  # False for NaN
    nalpha = np.where(above, alpha_of(nd, ada), alpha).astype(F32)
    cand = nd > delta  # a strict rise; False for NaN
    if cand.any():
        flat = np.where(cand, nd, -np.inf).ravel()
        i = int(np.argmax(flat))  # the first of equal maxima: the lowest row-major index
        if flat[i] > np.float32(md[0]):
            md = (float(flat[i]), int(first + i // cols), int(i % cols))
    return ndata, nd, nalpha, md


def md_bytes(md):
    return np.float32(md[0]).tobytes() + np.array([md[1], md[2]], "<i4").tobytes()


# ---- pieces: shapes, push sets, row maps -----------------------------------------------------
ROWS = 157
FIRST = 7  # key of row 0 in the piece tests
# by R: 4 (NV 1, R 16), 8, 128 (512 vectors per wave exactly), 132 (R 15), 200 (R 10),
# 680 (R 3), 684 (R 2), 1020 (510 of 512 vectors)
WIDTHS = [4, 8, 128, 132, 200, 680, 684, 1020]
PUSH_SETS = ["one", "full3", "subset3"]
MANY_WIDTHS = [4, 200]  # 64 pushes
# (row_block, row_stride, row_off, ntask) per piece, each piece into a buffer of its own
S3 = (ROWS - 1 + 3) // 3  # 53: linearSplit's step for three shards; rows 157, 158 are padding
ROW_MAPS = {"whole": [(ROWS, ROWS, 0, ROWS)], "split3": [(27, S3, 0, 3 * 27), (26, S3, 27, 3 * 26)]}
UNLISTED = np.arange(5, ROWS, 7)  # rows no push of "subset3" lists


def padding_tasks(piece):
    """Task rows of a piece whose model row is at or beyond ROWS."""
    b, s, o, n = piece
    t = np.arange(n)
    return t[(t // b) * s + o + t % b >= ROWS]


def orders(rng, rows, push_set):
    asc = np.arange(rows)
    if push_set == "one":
        return [rng.permutation(rows)]
    if push_set == "full3":
        return [asc, rng.permutation(rows), rng.permutation(rows)]
    listed = np.setdiff1d(asc, UNLISTED[UNLISTED < rows])
    if push_set == "subset3":
        return [rng.permutation(listed)[: (2 * len(listed)) // 3] for _ in range(3)]
    if push_set == "many64":
        return [asc if b % 5 == 0 else rng.permutation(rows) if b % 5 < 3 else
                rng.permutation(listed)[: len(listed) // 2] for b in range(64)]
    raise KeyError(push_set)


def gradients(rng, n, cols, scale=1.0):
    return (rng.standard_normal((n, cols)) * scale).astype(F32)


def piece_pushes(cols, push_set, rows=ROWS, first=FIRST, seed=0):
    rng = np.random.default_rng([cols, len(push_set), seed])
    return [encode(first + o, gradients(rng, len(o), cols)) for o in orders(rng, rows, push_set)]


# ---- pieces: special values ---------------------------------------------------------------
SPECIAL_COLS = 8
SPECIALS = dict(minus_zero=(20, 3), denormal=(41, 0), mixed_denormal=(41, 5), inf=(77, 2), nan=(120, 6))


def special_pushes(first=FIRST):
    """Three permuted full-range pushes of small normals, except: row 20 is listed by push 1
    alone and holds -0.0 at (20, 3) there; (41, 0) gets a denormal in every push and (41, 5)
    a denormal in push 0 only; (77, 2) gets +Inf in push 1; (120, 6) the NaN in push 2."""
    cols = SPECIAL_COLS
    rng = np.random.default_rng(1234)
    tiny = np.finfo(np.float32).smallest_subnormal
    out = []
    for b in range(3):
        o = rng.permutation(ROWS)
        if b != 1:
            o = o[o != SPECIALS["minus_zero"][0]]
        g = gradients(rng, len(o), cols, 1e-2)
        at = {int(r): i for i, r in enumerate(o)}
        r, c = SPECIALS["denormal"]
        g[at[r], c] = tiny * np.float32((3, 500, -77)[b])
        if b == 0:
            r, c = SPECIALS["mixed_denormal"]
            g[at[r], c] = -tiny * np.float32(9)
        if b == 1:
            r, c = SPECIALS["minus_zero"]
            g[at[r], c] = -0.0
            r, c = SPECIALS["inf"]
            g[at[r], c] = np.inf
        if b == 2:
            r, c = SPECIALS["nan"]
            g.view(np.uint32)[at[r], c] = NAN_BITS
        out.append(encode(first + o, g))
    return out


def special_rule_holds(pushes, rows, cols, first=FIRST):
    """tests/opseq.py's rule: no element is handed two NaNs, none gets +Inf and -Inf (their sum
    would create a NaN), and no square or sum of the finite gradients overflows into one."""
    nans = np.zeros((rows, cols), np.int64)
    pinf = np.zeros((rows, cols), bool)
    ninf = np.zeros((rows, cols), bool)
    for p in pushes:
        keys, g = decode(p, cols)
        r = keys - first
        nans[r] += np.isnan(g)
        pinf[r] |= np.isposinf(g)
        ninf[r] |= np.isneginf(g)
    return bool((nans <= 1).all() and not (pinf & ninf).any())


# ---- pieces: failed handles ------------------------------------------------------------------
def failed_pushes(kind, cols, first=FIRST):
    """Three permuted full-range pushes; push 1 holds a key outside the matrix ('oos') or
    lists one row twice ('dup')."""
    rng = np.random.default_rng([cols, len(kind)])
    out = []
    for b in range(3):
        o = rng.permutation(ROWS)
        if b == 1 and kind == "oos":
            o[31] = ROWS + 5
        if b == 1 and kind == "dup":
            o[31] = o[90]
        out.append(encode(first + o, gradients(rng, ROWS, cols)))
    return out


def plain_pushes(cols, seed, first=FIRST):
    """Three permuted key-subset pushes of a plain f32 matrix and their ordered sum from zero."""
    rng = np.random.default_rng([cols, seed, 99])
    expect = np.zeros((ROWS, cols), F32)
    out = []
    for o in orders(rng, ROWS, "subset3"):
        g = gradients(rng, len(o), cols)
        expect[o] = expect[o] + g
        out.append(encode(first + o, g))
    return out, expect


# ---- pieces: the all-identity branch -----------------------------------------------------------
IDENT_ROWS, IDENT_COLS, IDENT_W = 2_200_000, 4, 2
IDENT_CASES = ["all_id", "mixed", "oos"]


def ident_table_bytes(rows=IDENT_ROWS, nb=IDENT_W):
    """full_range_beyond_caches' measure of a call's slot table."""
    return rows * slot_stride(nb) * 4


def ident_pushes(case):
    """Two full-range pushes, keys from 0: both ascending; the second rotated by one record;
    the second with one key outside the matrix."""
    rng = np.random.default_rng(len(case))
    out = []
    for b in range(IDENT_W):
        keys = np.arange(IDENT_ROWS)
        if b == 1 and case == "mixed":
            keys = np.roll(keys, 1)
        if b == 1 and case == "oos":
            keys[1_000_000] = IDENT_ROWS + 5
        out.append(encode(keys, rng.standard_normal((IDENT_ROWS, IDENT_COLS), dtype=np.float32)))
    return out


# ---- apply: general states -----------------------------------------------------------------------
APPLY_SHAPES = [(157, 200, 0), (157, 4, 0), (37, 1028, 0), (157, 8, 1000)]  # rows, cols, first key
ZERO_ROWS = slice(3, None, 9)  # rows of `apply_src` that are zero in both halves (unlisted)


def start_pushes(rows, cols, first, seed=0):
    """Three ordinary pushes (ascending, permuted, a key subset) whose squares sum to about 1:
    after them a good part of the deltas is above 1 and a good part is not."""
    rng = np.random.default_rng([rows, cols, seed])
    os_ = [np.arange(rows), rng.permutation(rows), rng.permutation(rows)[: rows // 2]]
    return [bytes(encode(first + o, gradients(rng, len(o), cols, 0.6))) for o in os_]


def apply_src(rows, cols, seed=0):
    """[rows, 2 * cols]: Σu of either sign, Σu² >= 0 with a part exactly 0 (no rise there);
    ZERO_ROWS all +0.0 except one -0.0 in Σu."""
    rng = np.random.default_rng([rows, cols, seed, 5])
    src = np.empty((rows, 2 * cols), F32)
    src[:, :cols] = gradients(rng, rows, cols, 0.3)
    sq = gradients(rng, rows, cols, 0.7)
    sq = (sq * sq).astype(F32)
    sq[rng.random((rows, cols)) < 0.2] = 0.0
    src[:, cols:] = sq
    src[ZERO_ROWS] = 0.0
    src[ZERO_ROWS.start, 0] = -0.0
    return src


# ---- apply: maxDelta ties (fresh store: delta 0, nd = Σu²) -----------------------------------------
# case -> (rows, cols, [(row, col), ...] holding the equal maxima, the winner)
TIES = {
    "vector": (157, 8, [(10, 6), (10, 4)], (10, 4)),                   # two elements of one 16-B vector
    "block": (157, 8, [(100, 2), (1, 5)], (1, 5)),                     # vectors 200 and 3: threads of block 0
    # cols 4: vector index = row. 256 * 5 + 3 is block 5's first trip, 2048 * 256 + 7 block 0's second
    "blocks": (524_300, 4, [(K_MOMENT_BLOCKS * 256 + 7, 1), (256 * 5 + 3, 2)], (256 * 5 + 3, 2)),
}
TIE_VALUE = np.float32(4.0)


def tie_src(case):
    rows, cols, at, _ = TIES[case]
    rng = np.random.default_rng(len(case))
    src = np.empty((rows, 2 * cols), F32)
    src[:, :cols] = rng.standard_normal((rows, cols), dtype=np.float32) * np.float32(1e-3)
    sq = rng.standard_normal((rows, cols), dtype=np.float32) * np.float32(1e-3)
    src[:, cols:] = sq * sq
    for r, c in at:
        src[r, cols + c] = TIE_VALUE
    return src


def single(rows, cols, elems):
    """A src that is +0.0 except Σu² = value at the named elements: [((row, col), value), ...]."""
    src = np.zeros((rows, 2 * cols), F32)
    for (r, c), v in elems:
        src[r, cols + c] = v
    return src


# ---- the setAlpha divergence ------------------------------------------------------------------------
NEW_ALPHA = (0.05, 0.0002, 2.0)


def set_alpha_push(rows, cols, first, seed=3):
    """One push that lists every row but ZERO_ROWS, and the src of the same update."""
    rng = np.random.default_rng([rows, cols, seed, 11])
    listed = np.setdiff1d(np.arange(rows), np.arange(rows)[ZERO_ROWS])
    o = rng.permutation(listed)
    g = gradients(rng, len(o), cols, 0.6)
    src = np.zeros((rows, 2 * cols), F32)
    src[o, :cols] = g
    src[o, cols:] = g * g
    return bytes(encode(first + o, g)), src, listed

"""The yardstick of the chained reduce-scatter of AdaGrad matrices
(dml_group_push_chained on a FloatMatrixStoreAdaGrad group,
dml_prereduce_chain_piece_ada, dml_store_assign_adagrad_device), beside
tests/chain_expect.py: what every shard must hold, byte for byte.

Shard s is one OracleStore(..., ada_grad=1) over the shard's key range, fed, call
after call, the pushes of rank s, then s+1, ..., then s-1 (chain_expect.rotated),
each in push order and restricted to the shard's records. After every call the
shard's data, delta, alpha and max_delta() are recorded; set_alpha may be applied
between calls, and pushes the owner applies on its own after a call.

Inputs: gradients whose per-column scale straddles 1 / sqrt(adds per element), so
that after every call a good part of the deltas is above 1 (alpha moves) and a
good part is not (alpha stays); tests/test_chain_ada_expect.py checks that.
"""
import numpy as np

import chain_expect as X

VT = 1  # FloatMatrixStoreAdaGrad: fp32
F32 = np.dtype("<f4")


def col_scale(cols, adds):
    """Per-column gradient scale: scale^2 * adds runs log-uniformly over [0.2, 20], so the
    share of deltas above 1 is about 0.4 after a third of the adds and 0.65 after all."""
    t = np.arange(cols) / max(cols - 1, 1)
    return np.sqrt(0.2 * 100.0 ** t / adds).astype(F32)


def pushes(rank, W, rows, cols, call, adds, asc=False, listed=None):
    """W pushes of `rank` for `call`, each listing every row of `listed` (default: all rows)
    once, ascending or in a seeded permuted order."""
    from distml_amd.store import encode_matrix_push
    listed = np.arange(rows) if listed is None else np.asarray(listed)
    sc = col_scale(cols, adds)
    out = []
    for b in range(W):
        r = np.random.default_rng(7000 * call + 100 * rank + b)
        keys = listed if asc else r.permutation(listed)
        vals = (r.standard_normal((len(keys), cols)).astype(F32) * sc).astype(F32)
        out.append(np.frombuffer(encode_matrix_push(keys, vals, 0, VT), np.uint8).copy())
    return out


def calls(world, W, rows, cols, ncalls, asc=False, short=lambda r, c: False, listed=None):
    adds = world * W * ncalls
    return [[[] if short(r, c) else pushes(r, W, rows, cols, c, adds, asc=asc, listed=listed) for r in range(world)]
            for c in range(ncalls)]


def edit(push, cols, row, col, value):
    """Sets the gradient of (row, col) in a push (uint8 array, in place); col None: the whole
    row. The row must be listed."""
    rec = push.reshape(-1, 4 + 4 * cols)
    keys = rec[:, :4].copy().view("<i4").ravel()
    i = int(np.flatnonzero(keys == row)[0])
    v = rec[i, 4:].copy().view(F32)
    if col is None:
        v[:] = value
    else:
        v[col] = value
    rec[i, 4:] = v.view(np.uint8)


def expected(oracle, world, rows, cols, calls_pushes, init, order=X.rotated, skip=lambda r, c: False,
             set_alpha={}, after=lambda s, c: [], orders={}):
    """[call][shard] -> dict(data, delta, alpha, md) after every call. set_alpha[c] = (initial,
    min, factor) is applied to every shard after call c; after(s, c): pushes shard s's owner
    applies itself right after call c (and after that set_alpha); orders[c]: call c's rank
    order where it is not `order` (a push_exchange call applies rank-major)."""
    out = [[None] * world for _ in calls_pushes]
    for s, (first, last) in enumerate(X.shard_ranges(world, rows)):
        o = oracle.OracleStore(1, 0, VT, first, last, cols, ada_grad=1)
        o.data[:] = init[first:last + 1]
        for c, per_rank in enumerate(calls_pushes):
            for r in orders.get(c, order)(world, s):
                if skip(r, c):
                    continue
                for p in per_rank[r]:
                    b = X.restrict(p, VT, cols, first, last)
                    if b:
                        assert o.push(b) == 0
            if c in set_alpha:
                o.set_alpha(*set_alpha[c])
            for p in after(s, c):
                assert o.push(bytes(p)) == 0
            out[c][s] = dict(data=np.array(o.data, copy=True), delta=np.array(o.delta, copy=True),
                             alpha=np.array(o.alpha, copy=True), md=o.max_delta())
        o.close()
    return out


def same_md(got, want) -> bool:
    """(value, row, col), the value by its bits."""
    return (X.same_bits(np.array([got[0]]), np.array([want[0]]), VT) and int(got[1]) == int(want[1])
            and int(got[2]) == int(want[2]))


def alpha_formula(delta, initial, minimum, factor):
    """(float)(initialAlpha / (factor * sqrt((double)delta))) clamped to minAlpha, the
    parameters taken as the floats the stores hold (FloatMatrixStoreAdaGrad.java:268-272)."""
    ia, mn, fa = (np.float64(np.float32(x)) for x in (initial, minimum, factor))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (ia / (fa * np.sqrt(delta.astype(np.float64)))).astype(F32)
    return np.where(a < np.float32(mn), np.float32(mn), a).astype(F32)


# ---- the maxDelta tie inputs ----------------------------------------------------------
# world 2, 40 x 8, two sub-chunks per slice: shard 1 = rows 20..39, its first piece rows
# 20..29, its second rows 30..39. Shard 1's ring order is rank 1, rank 0; rank-major is
# rank 0, rank 1. Every other gradient is ~1e-3 (deltas ~1e-5), the named elements get
# exactly 2.0 once and exactly 0.0 otherwise: they reach delta 4.0, the maximum.
TIE_WORLD, TIE_ROWS, TIE_COLS, TIE_W, TIE_PIECES = 2, 40, 8, 2, 2
TIE_B = (22, 3)  # first piece
TIE_A = (33, 5)  # second piece
TIE_Z = (36, 1)  # second piece
TIE_B2 = (24, 6)
TIE_A2 = (31, 2)


def tie_calls(case, asc):
    """case 'a': B through ring position 0's (rank 1's) push 1, A through ring position 1's
    (rank 0's) push 0: the holder is B (rank-major: A).
    case 'b': inside rank 1, A (second piece) through push 0 and B (first piece) through push
    1; rank 0 brings Z to 4.0 in its push 0: the holder is A (rank-major: Z).
    case 'c': call 0 is case 'a'; call 1 brings B2 and A2 to 4.0 the same way: the holder
    stays call 0's (ring: B; rank-major: A).
    Returns (calls, ring holder, rank-major holder)."""
    ncalls = 2 if case == "c" else 1
    named = [TIE_B, TIE_A, TIE_Z, TIE_B2, TIE_A2]
    cp = []
    for c in range(ncalls):
        per_rank = []
        for r in range(TIE_WORLD):
            ps = []
            for b in range(TIE_W):
                g = np.random.default_rng(50 * c + 10 * r + b)
                keys = np.arange(TIE_ROWS) if asc else g.permutation(TIE_ROWS)
                vals = (g.standard_normal((TIE_ROWS, TIE_COLS)) * 1e-3).astype(F32)
                from distml_amd.store import encode_matrix_push
                p = np.frombuffer(encode_matrix_push(keys, vals, 0, VT), np.uint8).copy()
                for (row, col) in named:
                    edit(p, TIE_COLS, row, col, 0.0)
                ps.append(p)
            per_rank.append(ps)
        cp.append(per_rank)

    def two(c, elem, rank, push):
        edit(cp[c][rank][push], TIE_COLS, elem[0], elem[1], 2.0)

    if case in ("a", "c"):
        two(0, TIE_B, 1, 1)
        two(0, TIE_A, 0, 0)
        ring, major = TIE_B, TIE_A
        if case == "c":
            two(1, TIE_B2, 1, 1)
            two(1, TIE_A2, 0, 0)
    elif case == "b":
        two(0, TIE_A, 1, 0)
        two(0, TIE_B, 1, 1)
        two(0, TIE_Z, 0, 0)
        ring, major = TIE_A, TIE_Z
    else:
        raise ValueError(case)
    return cp, ring, major


# ---- setAlpha and untouched rows ------------------------------------------------------
SET_ALPHA = (0.05, 1e-4, 2.0)
ZERO_ROW = 3  # listed by subset_pushes; its gradients are all +0.0 in call 1


def set_alpha_calls(world, W, rows, cols):
    """Call 0 lists every row (scaled gradients); call 1 is chain_expect.subset_pushes' row set
    (rows 5, 12, 19, ... unlisted) with the scaled gradients, ZERO_ROW's all +0.0."""
    listed = np.setdiff1d(np.arange(rows), np.arange(5, rows, 7))
    adds = world * W * 2
    c0 = [pushes(r, W, rows, cols, 0, adds) for r in range(world)]
    c1 = [pushes(r, W, rows, cols, 1, adds, listed=listed) for r in range(world)]
    for ps in c1:
        for p in ps:
            edit(p, cols, ZERO_ROW, None, 0.0)
    return [c0, c1]


# ---- special values --------------------------------------------------------------------
def special_calls(world, W, rows, cols):
    """Two calls over subset_pushes' row set from chain_expect.minus_zero_init (-0.0 in listed
    and unlisted rows). Call 0: one +Inf gradient. Call 1: one NaN gradient on each of two
    named elements of different shards, in the last columns (the largest scale: their delta
    is above 1 after call 0, so the alpha they hold before call 1 is a computed one).
    Returns (calls, inf element, the two NaN elements)."""
    listed = np.setdiff1d(np.arange(rows), np.arange(5, rows, 7))
    adds = world * W * 2
    cp = [[pushes(r, W, rows, cols, c, adds, listed=listed) for r in range(world)] for c in range(2)]
    rng = X.shard_ranges(world, rows)
    inf_el = (int(listed[len(listed) // 3]), 1)
    nan_els = [(int(listed[np.searchsorted(listed, rng[0][0] + 4)]), cols - 1),
               (int(listed[np.searchsorted(listed, rng[world - 1][0] + 9)]), cols - 2)]
    edit(cp[0][world - 1][0], cols, inf_el[0], inf_el[1], np.inf)
    edit(cp[1][0][W - 1], cols, nan_els[0][0], nan_els[0][1], np.nan)
    edit(cp[1][world - 1][1], cols, nan_els[1][0], nan_els[1][1], np.nan)
    return cp, inf_el, nan_els


def nan_alpha_mask(want_delta):
    """Elements left out of the alpha comparison: those whose delta came home NaN."""
    return np.isnan(want_delta)


# ---- the ring-order cases (tests/test_gpu_chain_ada.py), W = 5 per rank, two calls, rank 0
# passes nothing in call 1: (world, rows, cols, pieces, ascending, blocked row map)
RING_W, RING_CALLS = 5, 2
RING_CASES = [(3, 1198, 200, 1, True, False), (2, 999, 200, 4, True, True), (3, 1000, 64, 2, False, False),
              (4, 1000, 67, 1, False, False), (2, 300, 256, 2, True, False), (2, 300, 300, 1, False, False),
              (2, 300, 3, 1, False, False)]


def ring_calls(world, rows, cols, asc):
    return calls(world, RING_W, rows, cols, RING_CALLS, asc=asc, short=lambda r, c: (r, c) == (0, 1))


# ---- the native group's cases (tests/chain_ada_group_worker.py, test_native_chain_ada.py)
GROUP_W, GROUP_CALLS = 3, 3


def group_calls(world, rows, cols, asc):
    """Three calls; rank 0 passes no push in call 1."""
    return calls(world, GROUP_W, rows, cols, GROUP_CALLS, asc=asc, short=lambda r, c: (r, c) == (0, 1))


def fail_calls(world, rows, cols):
    """Three calls over subset_pushes' row set (rows 5, 12, ... unlisted), scaled gradients."""
    listed = np.setdiff1d(np.arange(rows), np.arange(5, rows, 7))
    return calls(world, GROUP_W, rows, cols, GROUP_CALLS, listed=listed)


def local_push(rank, first, last, cols, adds):
    """One push of the owner's own rows, descending keys (push_local between chained calls)."""
    from distml_amd.store import encode_matrix_push
    keys = np.arange(first, last + 1)[::-1]
    g = np.random.default_rng(900 + rank)
    vals = (g.standard_normal((len(keys), cols)).astype(F32) * col_scale(cols, adds)).astype(F32)
    return np.frombuffer(encode_matrix_push(keys, vals, 0, VT), np.uint8).copy()

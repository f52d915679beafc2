"""The yardstick of the chained int32 reduce-scatter (dml_group_push_chained_i32,
dml_prereduce_chain_piece_i32 / _close_i32): what every shard must hold, and which
error it must report.

Shard s of KeyRange(0, rows-1).linearSplit(world) is one reference IntMatrixStore (the
CPU oracle, value type int32) over that shard's key range, fed, call after call, the
pushes of rank s, then rank s+1, ..., then rank s-1 (chain_expect.rotated), each in push
order and restricted to the shard's records (chain_expect.restrict). A push that leaves a
counter negative returns non-zero (IntMatrixStore.java:174-176): the oracle then holds
every add up to and including that one, and the shard is fed nothing more, in that call
or any later one (PSAgent.java:188-191).

The module also holds the inputs of the GPU tests, so that tests/test_chain_i32_expect.py
can show, on the CPU, that the yardstick tells the cases apart.
"""
import numpy as np

import chain_expect as X

VT = 0  # DataDesc.ELEMENT_TYPE_INT
I4 = np.dtype("<i4")
# chain_expect's dtype tables, with the int32 entry restrict() needs
X.VDT.setdefault(VT, I4)
X.UDT.setdefault(VT, np.dtype("<u4"))

NEG = 4  # DML_E_NEGATIVE_COUNTER == ORC_E_NEGATIVE_COUNTER
INT_MAX = 2 ** 31 - 1


def init_counts(rows, cols):
    """Counts no clean case can drive negative: at least 1000, while the pushes' deltas are
    >= -2 and no element receives more than 192 adds in any test here (W = 64 at world 3,
    one call: -384 at worst). 64 + h % 51 would not survive 33 such adds."""
    h = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols) * 2654435761 % 51
    return (1000 + h).astype(I4)


def encode(keys, vals):
    from distml_amd.store import encode_matrix_push
    return np.frombuffer(encode_matrix_push(np.asarray(keys), np.ascontiguousarray(vals, I4), 0, VT), np.uint8).copy()


def decode(push, cols):
    rec = np.frombuffer(bytes(push), np.uint8).reshape(-1, 4 + 4 * cols)
    return rec[:, :4].copy().view("<i4").ravel(), rec[:, 4:].copy().view(I4).reshape(-1, cols)


def pushes(rank, W, rows, cols, call, kind="perm"):
    """W pushes of one rank and call, deltas in [-2, 3]. perm: every row once, seeded order;
    asc: every row, ascending keys; subset: a seeded third of the rows (LDA's touched rows),
    never rows 5, 12, 19, ..."""
    out = []
    for b in range(W):
        r = np.random.default_rng(100000 * call + 1000 * rank + b)
        if kind == "asc":
            keys = np.arange(rows)
        elif kind == "subset":
            listed = np.setdiff1d(np.arange(rows), np.arange(5, rows, 7))
            keys = r.permutation(listed)[: max(1, len(listed) // 3)]
        else:
            keys = r.permutation(rows)
        out.append(encode(keys, r.integers(-2, 4, size=(len(keys), cols))))
    return out


def calls_of(world, W, rows, cols, ncalls, kind="perm", short=lambda r, c: False):
    return [[[] if short(r, c) else pushes(r, W, rows, cols, c, kind) for r in range(world)] for c in range(ncalls)]


def poke(push, cols, key, col, value, at=None):
    """`push` with the value of (key, col) replaced; at: the record of `key` is first swapped
    to record position `at` (the push keeps listing every row once)."""
    keys, vals = decode(push, cols)
    i = int(np.flatnonzero(keys == key)[0])
    if at is not None and at != i:
        keys[[i, at]] = keys[[at, i]]
        vals[[i, at]] = vals[[at, i]]
        i = at
    vals[i, col] = value
    return encode(keys, vals)


def expected(oracle, world, rows, cols, calls_pushes, init, order=X.rotated, skip=lambda r, c: False,
             after=lambda s, c: [], orders=None):
    """Per shard: (values, (code, key, col)) of one oracle store fed calls_pushes[c][r] in the
    order order(world, s) gives, stopped for good at its first non-zero return. skip(r, c):
    rank r's call c adds nothing anywhere (a failed call); after(s, c): pushes shard s's owner
    applies locally right after call c (refused like any other once the shard is closed);
    orders: {call: order function} for calls that are not chained (push_exchange: rank-major)."""
    out = []
    for s, (first, last) in enumerate(X.shard_ranges(world, rows)):
        o = oracle.OracleStore(1, 0, VT, first, last, cols)
        o.data[:] = init[first:last + 1]
        closed = False
        for c, per_rank in enumerate(calls_pushes):
            ord_c = (orders or {}).get(c, order)
            feed = [p for r in ord_c(world, s) if not skip(r, c) for p in per_rank[r]]
            feed = [X.restrict(p, VT, cols, first, last) for p in feed] + [bytes(p) for p in after(s, c)]
            for b in feed:
                if closed or not b:
                    continue
                closed = o.push(b) != 0
        out.append((np.array(o.data, copy=True), o.error() if closed else (0, 0, -1)))
        o.close()
    return out


# ---- the error cases of tests/test_gpu_chain_i32.py: (calls, init) at world 3 -------------
WORLD, ROWS = 3, 1000
BIG = -100000  # an add no count here survives


def _base(cols, W=3, ncalls=1):
    return calls_of(WORLD, W, ROWS, cols, ncalls), init_counts(ROWS, cols)


def case_negative_at(cols, ring_step, shard=1):
    """The first negative of shard `shard` comes from the rank at ring step `ring_step` (0: its
    owner, 1: the middle rank, 2: the last), in its push 1, at row first + 40, column cols // 2.
    A second call follows: the closed shard must ignore it."""
    calls, init = _base(cols, ncalls=2)
    first, _ = X.shard_ranges(WORLD, ROWS)[shard]
    r = (shard + ring_step) % WORLD
    calls[0][r][1] = poke(calls[0][r][1], cols, first + 40, cols // 2, BIG)
    return calls, init


def case_two_ranks(cols, shard=1):
    """Ranks shard + 1 and shard + 2 would both fail in slice `shard`: the ring-earlier one in
    its last push, late in it; the ring-later one in its push 0, record 0 — a smaller (push,
    offset), and, for shard 1, the rank that comes first in rank-major order."""
    calls, init = _base(cols)
    first, _ = X.shard_ranges(WORLD, ROWS)[shard]
    a, b = (shard + 1) % WORLD, (shard + 2) % WORLD
    calls[0][a][2] = poke(calls[0][a][2], cols, first + 7, 0, BIG, at=ROWS - 3)
    calls[0][b][0] = poke(calls[0][b][0], cols, first + 300, cols - 1, BIG, at=0)
    return calls, init


def case_late_subchunk(cols, shard=0):
    """The earliest failing position lies in the slice's last quarter (its last sub-chunk at
    pieces 2 and 4): rank shard + 1, push 1, record 2. The rows of the first quarter get their
    adds of that push at later records, and those of push 2 later still: all rolled back."""
    calls, init = _base(cols)
    first, last = X.shard_ranges(WORLD, ROWS)[shard]
    r = (shard + 1) % WORLD
    calls[0][r][1] = poke(calls[0][r][1], cols, last - 5, cols - 1, BIG, at=2)
    return calls, init


def case_dip(cols, shard=2):
    """A counter that holds 1 gets -2 from the middle rank's push 0 (-1: the reference throws)
    and +9 from its push 1: the sum of all terms stays >= 0, a final-counter check is blind."""
    calls, init = _base(cols)
    first, _ = X.shard_ranges(WORLD, ROWS)[shard]
    r = (shard + 1) % WORLD
    row, col = first + 11, cols - 1
    init = init.copy()
    init[row, col] = 1
    for q in range(WORLD):
        for b in range(3):
            calls[0][q][b] = poke(calls[0][q][b], cols, row, col, 0)
    calls[0][r][0] = poke(calls[0][r][0], cols, row, col, -2)
    calls[0][r][1] = poke(calls[0][r][1], cols, row, col, 9)
    return calls, init


def case_int_max(cols, shard=0):
    """INT_MAX + 1 wraps to INT_MIN: negative, the reference throws."""
    calls, init = _base(cols)
    first, _ = X.shard_ranges(WORLD, ROWS)[shard]
    row, col = first + 3, 0
    init = init.copy()
    init[row, col] = INT_MAX
    for q in range(WORLD):
        for b in range(3):
            calls[0][q][b] = poke(calls[0][q][b], cols, row, col, 0)
    calls[0][(shard + 2) % WORLD][1] = poke(calls[0][(shard + 2) % WORLD][1], cols, row, col, 1)
    return calls, init


# ---- the inputs of tests/test_native_chain_i32.py (W = 3 pushes per rank, 3 calls) ---------
GROUP_W, GROUP_CALLS = 3, 3


def group_calls(world, rows, cols, case):
    """chain: clean, rank 0 passes no push in call 1. close: call 0's first negative of shard 1
    comes from the rank after its owner (a middle rank from world 3 on). order: rank 1's own
    push 1 of call 0 closes its own shard (ring step 0). fail: world 3, rank 1's push closes
    shard 0 in call 0 — the call in which rank 2 hands over a truncated push."""
    short = (lambda r, c: (r, c) == (0, 1)) if case == "chain" else (lambda r, c: False)
    calls = calls_of(world, GROUP_W, rows, cols, GROUP_CALLS, short=short)
    rng = X.shard_ranges(world, rows)
    if case == "close":
        r = 2 % world
        calls[0][r][1] = poke(calls[0][r][1], cols, rng[1][0] + 40, cols // 2, BIG)
    elif case == "order":
        calls[0][1][1] = poke(calls[0][1][1], cols, rng[1][0] + 40, cols // 2, BIG)
    elif case == "fail":
        calls[0][1][0] = poke(calls[0][1][0], cols, rng[0][0] + 17, cols - 1, BIG)
    return calls


def local_push(rank, first, last, cols):
    """One push of the rank's own rows, descending keys (the order-with-other-calls case)."""
    keys = np.arange(first, last + 1)[::-1]
    return encode(keys, np.random.default_rng(770 + rank).integers(-2, 4, size=(len(keys), cols)))

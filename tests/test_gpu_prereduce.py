"""GPU, one process: the pre-reduce engine's three entries, end to end.

dml_prereduce_begin (a pooled workspace lease), dml_prereduce_begin_ctx (a speculative
context's workspace ring) and dml_reduce_buckets_dense, through distml_amd.group.HipOps.
Every partial is compared byte for byte with the ordered sum from zero computed in numpy:
one rounding per add, in push order (int32 wraps).

Shapes, by the dispatch branch a handle's pieces take (dml_kernels.hip: spec_shape,
use_flat, launch_auto):
  f32 64 x 1024  whole 4-KiB rows, a speculation shape      k_reduce_rows FULL
  f32 96 x 64    flat rows, a speculation shape             k_reduce_flat / k_flat_ident
  f32 96 x 67    ragged rows, no speculation                k_reduce_rows pair-packed
  f64 64 x 33    ragged fp64 rows                           k_reduce_rows pair-packed
  i32 64 x 48    flat int32 rows                            k_reduce_flat / k_flat_ident
Push sets: three ascending pushes; the middle one permuted; the last one listing half the
rows (no longer full-range: a context call then does not speculate).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VDT = {0: np.int32, 1: np.float32, 3: np.float64}
FIRST = 7  # key of row 0
SHAPES = [(1, 64, 1024), (1, 96, 64), (1, 96, 67), (3, 64, 33), (0, 64, 48)]
PUSH_SETS = ["ascending", "permuted", "half"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _values(rng, vt, n, cols):
    if vt == 0:
        return rng.integers(-1000, 1000, size=(n, cols), dtype=np.int32)
    return rng.standard_normal((n, cols)).astype(VDT[vt])


def _push(vt, rows_listed, values):
    """One encoded push (device bytes) listing `rows_listed` in that order."""
    from distml_amd import encode_matrix_push
    raw = encode_matrix_push(np.asarray(rows_listed) + FIRST, values, 0, vt)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


def _make_call(rng, vt, rows, cols, orders, base=None):
    """Pushes listing the rows of `orders` (one array of distinct rows per push) and the
    ordered sum they give, from zero or from `base`."""
    expect = np.zeros((rows, cols), VDT[vt]) if base is None else base.copy()
    dev = []
    for order in orders:
        v = _values(rng, vt, len(order), cols)
        expect[order] += v  # distinct rows: one rounding per add, push order
        dev.append(_push(vt, order, v))
    return dev, expect


def _orders(rng, rows, push_set):
    asc = np.arange(rows)
    if push_set == "ascending":
        return [asc, asc, asc]
    if push_set == "permuted":
        return [asc, rng.permutation(rows), asc]
    return [asc, asc, rng.permutation(rows)[: rows // 2]]


def _args(dev):
    return [d.data_ptr() for d in dev], [d.numel() for d in dev]


def _run_pieces(ops, h, vt, rows, cols, out, stream, npieces=2):
    per = rows // npieces
    rowb = cols * VDT[vt]().itemsize
    for j in range(npieces):
        ops.piece(h, per, per, j * per, per, out.data_ptr() + j * per * rowb, stream)


def _fresh(vt, rows, cols):
    """An output buffer no route leaves as it found it."""
    return torch.full((rows * cols,), 7, dtype={0: torch.int32, 1: torch.float32, 3: torch.float64}[vt], device="cuda")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _plain_call(ops, fmt, vt, rows, cols, dev, side):
    """dml_prereduce_begin, two pieces of half the rows each on a side stream, _end."""
    out = _fresh(vt, rows, cols)
    torch.cuda.synchronize()
    ptrs, lens = _args(dev)
    h = ops.begin(fmt, FIRST, rows, cols, ptrs, lens, torch.cuda.current_stream().cuda_stream)
    try:
        _run_pieces(ops, h, vt, rows, cols, out, side.cuda_stream)
        side.synchronize()
    finally:
        ops.end(h)
    return out


def _ctx_call(ops, ctx, vt, rows, cols, dev, side):
    """dml_prereduce_begin_ctx, the same pieces, _verify, _end. Returns (partial, re-ran)."""
    out = _fresh(vt, rows, cols)
    torch.cuda.synchronize()
    ptrs, lens = _args(dev)
    h = ops.begin_ctx(ctx, ptrs, lens, torch.cuda.current_stream().cuda_stream)
    rerun = None
    try:
        _run_pieces(ops, h, vt, rows, cols, out, side.cuda_stream)
        rerun = ops.verify(h)
    finally:
        ops.end(h)
    torch.cuda.synchronize()
    return out, rerun


@pytest.mark.parametrize("push_set", PUSH_SETS)
@pytest.mark.parametrize("vt,rows,cols", SHAPES)
def test_three_entries_agree(vt, rows, cols, push_set):
    """begin + pieces, begin_ctx + pieces + verify, and dml_reduce_buckets_dense give the
    same bytes, and those are the ordered sum from zero."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    ops, fmt = HipOps(), DataDesc(1, 0, vt)
    rng = np.random.default_rng(1000 * vt + cols + len(push_set))
    dev, expect = _make_call(rng, vt, rows, cols, _orders(rng, rows, push_set))
    side = torch.cuda.Stream()
    a = _plain_call(ops, fmt, vt, rows, cols, dev, side)
    ctx = ops.ctx_create(fmt, FIRST, rows, cols, 0)
    try:
        b, _ = _ctx_call(ops, ctx, vt, rows, cols, dev, side)
    finally:
        ops.ctx_destroy(ctx)
    c = _fresh(vt, rows, cols)
    torch.cuda.synchronize()
    ptrs, lens = _args(dev)
    ops.prereduce(fmt, FIRST, rows, cols, ptrs, lens, c.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = expect.tobytes()
    assert _bytes(a) == want, "begin + pieces"
    assert _bytes(b) == want, "begin_ctx + pieces + verify"
    assert _bytes(c) == want, "dml_reduce_buckets_dense"


def test_context_counters():
    """dml_prectx_stats after each call of a context on f32 96 x 64.

    Call 0 lists every row in order twice: one speculative chunk, two identity pushes, and
    both pieces go through k_flat_ident (ident_launches). Calls 1-4 pass an ascending push
    and the same permutation: the ascending push is identity every time; the permutation is
    indexed in calls 1-3 (their workspaces of the ring of three hold no verified permutation
    yet: two are fresh, the third kept call 0's table, which has none) and reused in call 4,
    whose workspace call 1 left with the permutation's column kept. Call 5 passes a push that
    repeats a row: its speculation fails, the call re-runs exactly (both pushes indexed), the
    re-run's index sees the repeat and _end refuses the call."""
    from distml_amd import DataDesc, NativeError
    from distml_amd._lib import DML_E_UNSUPPORTED
    from distml_amd.group import HipOps
    vt, rows, cols = 1, 96, 64
    ops, fmt = HipOps(), DataDesc(1, 0, vt)
    rng = np.random.default_rng(96)
    asc, perm = np.arange(rows), rng.permutation(rows)
    side = torch.cuda.Stream()
    zero = dict(chunks=0, spec_chunks=0, spec_reruns=0, identity_pushes=0, reused_pushes=0, indexed_pushes=0,
                sparse_big_chunks=0, sparse_replays=0, ident_launches=0)
    steps = [([asc, asc], dict(chunks=1, spec_chunks=1, identity_pushes=2, ident_launches=2))]
    for i in range(1, 4):
        steps.append(([asc, perm], dict(chunks=1 + i, spec_chunks=1 + i, identity_pushes=2 + i, indexed_pushes=i,
                                        ident_launches=2)))
    steps.append(([asc, perm], dict(chunks=5, spec_chunks=5, identity_pushes=6, indexed_pushes=3, reused_pushes=1,
                                    ident_launches=2)))
    ctx = ops.ctx_create(fmt, FIRST, rows, cols, 0)
    try:
        assert ops.ctx_stats(ctx) == zero
        for i, (orders, counters) in enumerate(steps):
            dev, expect = _make_call(rng, vt, rows, cols, orders)
            out, rerun = _ctx_call(ops, ctx, vt, rows, cols, dev, side)
            assert not rerun, i
            assert _bytes(out) == expect.tobytes(), i
            assert ops.ctx_stats(ctx) == {**zero, **counters}, i
        dup = rng.permutation(rows)
        dup[5] = dup[50]  # one push lists a row twice
        dev = [_push(vt, o, _values(rng, vt, rows, cols)) for o in (asc, dup)]
        with pytest.raises(NativeError) as ei:
            _ctx_call(ops, ctx, vt, rows, cols, dev, side)
        assert ei.value.code == DML_E_UNSUPPORTED and str(ei.value) == "pre-reduce: a push repeats a row"
        assert ops.ctx_stats(ctx) == {**zero, **dict(chunks=6, spec_chunks=6, spec_reruns=1, identity_pushes=6,
                                                     indexed_pushes=5, reused_pushes=1, ident_launches=2)}
    finally:
        ops.ctx_destroy(ctx)


def test_lease_cleanliness_across_sizes_and_failures():
    """Plain handles draw their workspace from a per-device pool and hand it back marked
    clean or not; a lease serves any model that fits. One process, f32 x 64: a clean
    96-row call; a 40-row call with a key outside the matrix (refused at _end); 96 rows
    permuted; 40 rows clean; a chained call of ascending full-range pushes, whose late
    identity check leaves the slots the index filled unread; 96 rows permuted again."""
    from distml_amd import ArrayIndexOutOfBoundsException, DataDesc
    from distml_amd._lib import DML_E_KEY_OUT_OF_SHARD
    from distml_amd.group import HipOps
    vt, cols = 1, 64
    ops, fmt = HipOps(), DataDesc(1, 0, vt)
    rng = np.random.default_rng(4096)
    side = torch.cuda.Stream()

    def exact(rows, orders, what):
        dev, expect = _make_call(rng, vt, rows, cols, orders)
        assert _bytes(_plain_call(ops, fmt, vt, rows, cols, dev, side)) == expect.tobytes(), what

    exact(96, [np.arange(96), np.arange(96)], "96 rows, clean")
    bad = np.arange(40)
    bad[17] = 40 + 5  # row index past the matrix
    dev = [_push(vt, o, _values(rng, vt, 40, cols)) for o in (np.arange(40), bad)]
    with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
        _plain_call(ops, fmt, vt, 40, cols, dev, side)
    assert ei.value.code == DML_E_KEY_OUT_OF_SHARD and str(ei.value) == "pre-reduce: key outside the matrix"
    exact(96, [rng.permutation(96), np.arange(96), rng.permutation(96)], "96 rows permuted, after the failed call")
    exact(40, [np.arange(40), np.arange(40)], "40 rows, clean")
    # the chained call: out = base + the pushes' rows, in push order
    rows = 96
    base = _values(rng, vt, rows, cols)
    dev, expect = _make_call(rng, vt, rows, cols, [np.arange(rows), np.arange(rows)], base=base)
    dbase = torch.from_numpy(base.reshape(-1)).cuda()
    out = _fresh(vt, rows, cols)
    torch.cuda.synchronize()
    ptrs, lens = _args(dev)
    h = ops.begin(fmt, FIRST, rows, cols, ptrs, lens, torch.cuda.current_stream().cuda_stream)
    try:
        ops.chain_piece(h, rows, rows, 0, rows, dbase.data_ptr(), out.data_ptr(), side.cuda_stream)
        side.synchronize()
    finally:
        ops.end(h)
    assert _bytes(out) == expect.tobytes(), "chained call"
    exact(96, [rng.permutation(96), rng.permutation(96)], "96 rows permuted, after the chained call")


def test_timing_sample_counts_every_piece():
    """dml_prereduce_timing(1): each of three pieces on a plain handle, and of three on a
    context handle, adds one launch to dml_prereduce_kernel_time."""
    from distml_amd import DataDesc, _lib
    from distml_amd.group import HipOps
    vt, rows, cols = 1, 96, 64
    ops, fmt, L = HipOps(), DataDesc(1, 0, vt), _lib.load()
    rng = np.random.default_rng(3)
    dev, expect = _make_call(rng, vt, rows, cols, [np.arange(rows), rng.permutation(rows)])
    ptrs, lens = _args(dev)
    side = torch.cuda.Stream()

    def launches():
        ms, n = C.c_double(), C.c_int64()
        assert L.dml_prereduce_kernel_time(C.byref(ms), C.byref(n), 0) == 0
        return n.value

    ctx = ops.ctx_create(fmt, FIRST, rows, cols, 0)
    assert L.dml_prereduce_timing(1) == 0
    try:
        n0 = launches()
        out = _fresh(vt, rows, cols)
        torch.cuda.synchronize()
        h = ops.begin(fmt, FIRST, rows, cols, ptrs, lens, torch.cuda.current_stream().cuda_stream)
        try:
            _run_pieces(ops, h, vt, rows, cols, out, side.cuda_stream, npieces=3)
            side.synchronize()
        finally:
            ops.end(h)
        assert launches() == n0 + 3
        assert _bytes(out) == expect.tobytes()
        out = _fresh(vt, rows, cols)
        torch.cuda.synchronize()
        h = ops.begin_ctx(ctx, ptrs, lens, torch.cuda.current_stream().cuda_stream)
        try:
            _run_pieces(ops, h, vt, rows, cols, out, side.cuda_stream, npieces=3)
            ops.verify(h)
        finally:
            ops.end(h)
        assert launches() == n0 + 6
        torch.cuda.synchronize()
        assert _bytes(out) == expect.tobytes()
    finally:
        assert L.dml_prereduce_timing(0) == 0  # process-global
        ops.ctx_destroy(ctx)

"""GPU, one process: the chained reduce-scatter's building blocks.

dml_prereduce_chain_piece (HipOps.chain_piece): the ring is emulated with N
pre-reduce handles, one per virtual rank; every shard's slice walks the ranks
s, s+1, ..., s-1 in a host loop, each rank's piece adding its pushes' rows of the
slice, and the result is compared byte for byte (unsigned view) with
tests/chain_expect.py — the oracle fed that order.
dml_store_assign_dense_device (HipOps.assign): push, assign, push on a store
without and with the speculative second buffer.

Which kernel family a case reaches follows from the dispatch in
dml_kernels.hip (launch_reduce: use_flat() takes rows under 4 KiB of whole 16-B
vectors whose pushes list at least half the rows; launch_auto picks k_reduce for
rows narrower than one vector and a k_reduce_rows shape by width otherwise) and
from dml_prereduce_chain_piece (ascending full-range pushes of a flat shape are
verified key by key before the pieces, which then run k_flat_ident where the
host has waited for the index and no wave straddles two row blocks):
  f32 1000 x 64, f64 1000 x 64  permuted pushes, flat shape      k_reduce_flat
  f32 1000 x 67, f64 1000 x 67  ragged rows                      k_reduce_rows (pair-packed, 1 chunk)
  f32 1198 x 200 ascending      one row block per piece          k_flat_ident
  f32  999 x 200 ascending      125-row blocks, 10-row waves     k_reduce_flat with slot = row (the fallback)
  f32  300 x 256 ascending      1-KiB rows are a flat shape too  k_flat_ident
  f32   64 x 1024               whole 4-KiB rows                 k_reduce_rows FULL, 4 chunks per wave
  f32  300 x 3                  narrower than one vector         k_reduce
The -0.0 test adds pushes that list a third of the rows (use_flat() declines them), which
sends rows under 4 KiB to k_reduce_rows' other shapes: 256 and 512 columns (FULL, 1 and 2
chunks per wave), 300 (pair-packed, 2 chunks), fp64 128 columns (FULL, 1 chunk); and
1100 columns (pair-packed, 4 chunks, 2 chunk groups per row).
"""
import numpy as np
import pytest

import chain_expect as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run_ring(vt, world, rows, cols, pieces, calls, init, blocked=False, inplace=True, end_errors=None):
    """Every call: one handle per virtual rank (all its pushes, whole model), then slice s
    through ranks s, s+1, ..., s-1. pieces: sub-chunks per slice, one chain piece each —
    or, blocked, one piece per slice whose row map has `pieces` row blocks. Returns the
    shards' bytes as arrays."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    ops, fmt = HipOps(), DataDesc(1, 0, vt)
    rowb = cols * X.VDT[vt].itemsize
    ranges = X.shard_ranges(world, rows)
    shard = [_dev(init[f:l + 1]) for f, l in ranges]
    side = torch.cuda.Stream()
    keep = []
    for c, per_rank in enumerate(calls):
        dev = [[_dev(p) for p in per_rank[r]] for r in range(world)]
        keep.append(dev)
        torch.cuda.synchronize()
        hs = [ops.begin(fmt, 0, rows, cols, [d.data_ptr() for d in dev[r]], [d.numel() for d in dev[r]], 0)
              for r in range(world)]
        for s, (first, last) in enumerate(ranges):
            n = last - first + 1
            per = (n + pieces - 1) // pieces
            cur = shard[s]
            for t in range(world):
                h = hs[(s + t) % world]
                out = cur if inplace else torch.empty_like(cur)
                if blocked:
                    ops.chain_piece(h, per, per, first, n, cur.data_ptr(), out.data_ptr(), side.cuda_stream)
                else:
                    for r0 in range(0, n, per):
                        nr = min(per, n - r0)
                        ops.chain_piece(h, nr, nr, first + r0, nr, cur.data_ptr() + r0 * rowb,
                                        out.data_ptr() + r0 * rowb, side.cuda_stream)
                keep.append(cur)
                cur = out
            shard[s] = cur
        side.synchronize()
        for r, h in enumerate(hs):
            try:
                ops.end(h)
            except Exception as e:
                if end_errors is None:
                    raise
                end_errors.append((c, r, type(e).__name__))
    torch.cuda.synchronize()
    return [sh.cpu().numpy().view(X.VDT[vt]).reshape(-1, cols) for sh in shard]


# (vt, world, rows, cols, pieces, ascending, blocked)
CASES = [(1, 3, 1000, 64, 2, False, False), (1, 4, 1000, 67, 1, False, False), (1, 3, 1198, 200, 1, True, False),
         (1, 2, 999, 200, 4, True, True), (3, 3, 1000, 64, 2, False, False), (3, 2, 1000, 67, 1, False, False),
         (1, 2, 300, 256, 2, True, False), (1, 2, 64, 1024, 1, True, False), (1, 2, 300, 3, 1, True, False)]


@pytest.mark.parametrize("vt,world,rows,cols,pieces,asc,blocked", CASES)
def test_chain_pieces_match_the_ring_order(oracle, vt, world, rows, cols, pieces, asc, blocked):
    """Two calls of W = 3 pushes per rank (call 1: rank 0 passes none), every shard
    bytes-equal to the oracle fed the ring order."""
    W, ncalls = 3, 2
    calls = X.chain_calls(oracle, vt, world, rows, cols, W, ncalls, asc=asc, short=lambda r, c: (r, c) == (0, 1))
    init = X.init_values(vt, rows, cols)
    got = run_ring(vt, world, rows, cols, pieces, calls, init, blocked=blocked)
    want = X.expected_shards(oracle, vt, world, rows, cols, calls, init=init)
    for s in range(world):
        assert X.same_bits(got[s], want[s], vt), (s, int((X.bits(got[s], vt) != X.bits(want[s], vt)).sum()))


@pytest.mark.parametrize("vt,cols,asc", [(1, 64, False), (1, 67, False), (1, 200, True), (3, 64, False)])
def test_chain_in_place_equals_out_of_place(oracle, vt, cols, asc):
    world, rows = 3, 1000 if not asc else 1198
    calls = X.chain_calls(oracle, vt, world, rows, cols, 3, 1, asc=asc)
    init = X.init_values(vt, rows, cols)
    a = run_ring(vt, world, rows, cols, 2, calls, init, inplace=True)
    b = run_ring(vt, world, rows, cols, 2, calls, init, inplace=False)
    want = X.expected_shards(oracle, vt, world, rows, cols, calls, init=init)
    for s in range(world):
        assert X.same_bits(a[s], b[s], vt) and X.same_bits(a[s], want[s], vt), s


@pytest.mark.parametrize("vt,cols,sparse", [(1, 64, False), (1, 67, False), (3, 64, False), (1, 3, False),
                                            (1, 256, True), (1, 512, True), (1, 300, True), (3, 128, True),
                                            (1, 1100, False)])
def test_chain_minus_zero_and_pass_through(oracle, vt, cols, sparse):
    """-0.0 survives where nothing is added: rows no push lists (init -0.0 stays -0.0, an
    add of +0.0 would clear the sign), a handle with no pushes, and a handle whose index
    found a key outside the matrix (its _end raises, its pieces add nothing). Listed rows
    holding -0.0 get the oracle's sums, pushes of +-0.0 included."""
    from distml_amd.store import encode_matrix_push
    world, rows = 3, 240
    rng = np.random.default_rng(11)
    init = X.init_values(vt, rows, cols).copy()
    unlisted = np.setdiff1d(np.arange(rows), np.arange(1, rows, 3)) if sparse else np.arange(5, rows, 7)
    init[unlisted[::2]] = -0.0
    init[np.arange(3, rows, 11)] = -0.0  # listed rows
    listed = np.setdiff1d(np.arange(rows), unlisted)

    def push(seed, bad=False):
        r = np.random.default_rng(seed)
        keys = r.permutation(listed)
        vals = (r.standard_normal((len(keys), cols)) * 1e-3).astype(X.VDT[vt])
        vals[::5] = -0.0
        vals[1::5] = 0.0
        if bad:
            keys = keys.copy()
            keys[len(keys) // 2] = rows + 3  # outside the matrix
        return np.frombuffer(encode_matrix_push(keys, vals, 0, vt), np.uint8).copy()

    # call 0: every rank pushes; call 1: rank 1 passes nothing, rank 2's push 1 has a bad key
    calls = [[[push(10 * r + b) for b in range(2)] for r in range(world)],
             [[push(100), push(101)], [], [push(120), push(121, bad=True)]]]
    errs = []
    got = run_ring(vt, world, rows, cols, 2, calls, init, end_errors=errs)
    assert errs == [(1, 2, "ArrayIndexOutOfBoundsException")], errs
    want = X.expected_shards(oracle, vt, world, rows, cols, calls, init=init, skip=lambda r, c: (r, c) == (2, 1))
    neg0 = X.bits(np.array([-0.0]), vt)[0]
    for s, (f, l) in enumerate(X.shard_ranges(world, rows)):
        assert X.same_bits(got[s], want[s], vt), s
        mine = unlisted[::2][(unlisted[::2] >= f) & (unlisted[::2] <= l)] - f
        assert len(mine) and (X.bits(got[s], vt)[mine] == neg0).all(), s
    del rng


def test_chain_piece_refuses_int32_adagrad_and_speculative_handles(oracle):
    from distml_amd import DataDesc, _lib
    from distml_amd.group import HipOps
    from distml_amd.store import NativeError
    ops = HipOps()
    rows, cols = 64, 8
    buf = torch.zeros(rows * cols * 8, dtype=torch.uint8, device="cuda")
    for fmt in (DataDesc(1, 0, 0), DataDesc(1, 0, 1, False, True, True)):
        p = _dev(oracle.synth_dense_bucket(0, fmt.valueType, 0, rows, rows, cols, 3, 1, 0))
        torch.cuda.synchronize()
        h = ops.begin(fmt, 0, rows, cols, [p.data_ptr()], [p.numel()], 0)
        with pytest.raises(NativeError) as ei:
            ops.chain_piece(h, rows, rows, 0, rows, buf.data_ptr(), buf.data_ptr(), 0)
        assert ei.value.code == _lib.DML_E_UNSUPPORTED and "dml_group_push_exchange" in str(ei.value)
        ops.end(h)
    fmt = DataDesc(1, 0, 1)
    ctx = ops.ctx_create(fmt, 0, rows, cols, 0)
    p = _dev(oracle.synth_dense_bucket(0, 1, 0, rows, rows, cols, 3, 1, 0))
    torch.cuda.synchronize()
    h = ops.begin_ctx(ctx, [p.data_ptr()], [p.numel()], 0)
    with pytest.raises(NativeError) as ei:
        ops.chain_piece(h, rows, rows, 0, rows, buf.data_ptr(), buf.data_ptr(), 0)
    assert ei.value.code == _lib.DML_E_UNSUPPORTED
    ops.end(h)
    ops.ctx_destroy(ctx)


@pytest.mark.parametrize("vt,cols,second", [(1, 67, False), (1, 64, True), (3, 64, True), (0, 64, False)])
def test_store_assign_between_pushes(oracle, vt, cols, second):
    """dml_store_assign_dense_device: push, assign, push, read back = oracle(assigned value
    + second push). cols 67 is no speculation shape (spec_shape: whole 16-B vectors under
    4 KiB, or whole 4-KiB rows), so the store has one buffer; at 64 columns full-range
    pushes run speculatively and commit the store's second buffer (its value pointer moves
    after the first push — asserted), and the assign must land in the current one. int32
    stores check every add and never speculate: one buffer."""
    from distml_amd import DataDesc, DataStore, KeyRange
    from distml_amd.group import HipOps
    rows = 500
    fmt = DataDesc(1, 0, vt)
    st = DataStore(fmt, KeyRange(0, rows - 1), cols, async_push=True)
    dt = st.dtype
    rng = np.random.default_rng(3)
    init = (rng.integers(50, 60, size=(rows, cols)) if vt == 0 else rng.standard_normal((rows, cols))).astype(dt)
    st.load_values(init)
    p0 = st.device_ptr()
    a = _dev(oracle.synth_dense_bucket(0, vt, 0, rows, rows, cols, 21, 7, 3))
    b = _dev(oracle.synth_dense_bucket(0, vt, 0, rows, rows, cols, 22, 3, 1))
    val = (rng.integers(50, 60, size=(rows, cols)) if vt == 0 else rng.standard_normal((rows, cols))).astype(dt)
    if vt != 0:
        val[::9] = -0.0
    src = _dev(val)
    torch.cuda.synchronize()
    st.pushDevice([a.data_ptr()], [a.numel()])
    HipOps().assign(st, src.data_ptr(), rows * cols)
    st.pushDevice([b.data_ptr()], [b.numel()])
    st.flush()
    got = st.values()
    moved = st.device_ptr() != p0
    o = oracle.OracleStore(1, 0, vt, 0, rows - 1, cols)
    o.data[:] = val
    assert o.push(b.cpu().numpy().tobytes()) == 0
    assert got.tobytes() == o.data.tobytes()
    with pytest.raises(Exception):
        HipOps().assign(st, src.data_ptr(), rows * cols - 1)
    st.close()
    if second:
        # two speculative pushes: the value pointer moved twice (back to p0) or once; what
        # matters is that the second buffer existed while the assign ran
        st2 = DataStore(fmt, KeyRange(0, rows - 1), cols, async_push=True)
        q0 = st2.device_ptr()
        st2.pushDevice([a.data_ptr()], [a.numel()])
        st2.flush()
        assert st2.device_ptr() != q0
        st2.close()
    else:
        assert not moved

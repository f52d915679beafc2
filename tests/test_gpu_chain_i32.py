"""GPU, one process: the chained int32 reduce-scatter's building blocks.

The ring is emulated as tests/test_gpu_chain.py emulates the float one: one pre-reduce
handle per virtual rank and call; shard s's slice ([32-byte record][rows]) walks the
ranks s, s+1, ..., s-1 in a host loop, every step `pieces` HipOps.chain_piece_i32 and one
HipOps.chain_close_i32, and the owner (one int32 DataStore per shard) commits what comes
home with HipOps.assign_i32. Step 0 reads the store's rows and writes the slice buffer
(out != base); later steps run in place. Values and (code, key, col) are compared with
tests/chain_i32_expect.py, byte for byte.

Row widths and the instantiation of kChainCheckI32 each reaches (launch_auto):
  1024  k_reduce_rows FULL, 4 chunks      1000  pair-packed, 4 chunks
   512  k_reduce_rows FULL, 2 chunks       520  pair-packed, 2 chunks
   256  k_reduce_rows FULL, 1 chunk         67  pair-packed, 1 chunk
     3  k_reduce (narrower than one vector)
1 000 rows at world 3: shards of 334, 334 and 332 rows (a short last one).
"""
import struct

import numpy as np
import pytest

import chain_expect as X
import chain_i32_expect as E

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REC = 32
OPEN = b"\xff" * REC


def _dev(a):
    return torch.from_numpy(np.require(a, requirements=["C", "W"]).view(np.uint8).reshape(-1)).cuda()


def _rec(t):
    """(pos, key, col, step) of a record tensor; pos None = open."""
    pos, key, col, step = struct.unpack("<QqiI", bytes(t.cpu().numpy().tobytes())[:24])
    return (None if pos == 2 ** 64 - 1 else pos), key, col, step


def _values(st):
    """The store's values; a verdict the store had not retired yet surfaces once, on the way."""
    from distml_amd.store import IllegalStateException
    try:
        return st.values()
    except IllegalStateException:
        return st.values()


def run_ring(world, rows, cols, pieces, calls, init, end_errors=None, records=None):
    """Returns per shard (values, (code, key, col)) as the stores hold them after every call.
    records: list that receives (call, shard, record) of every slice as it came home."""
    from distml_amd import DataDesc, DataStore, KeyRange
    from distml_amd.group import HipOps
    from distml_amd.store import IllegalStateException
    ops, fmt = HipOps(), DataDesc(1, 0, E.VT)
    rowb = cols * 4
    ranges = X.shard_ranges(world, rows)
    stores = []
    for f, l in ranges:
        st = DataStore(fmt, KeyRange(f, l), cols, async_push=True)
        st.load_values(init[f:l + 1])
        stores.append(st)
    srec = [_dev(np.frombuffer(OPEN, np.uint8)) for _ in ranges]  # what each store's record holds
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
            known_closed = _rec(srec[s])[0] is not None
            buf = torch.empty(REC + n * rowb, dtype=torch.uint8, device="cuda")
            buf[:REC] = srec[s]
            torch.cuda.synchronize()
            shard_ptr = stores[s].device_ptr()
            rec_ptr, rows_ptr = buf.data_ptr(), buf.data_ptr() + REC
            for t in range(world):
                h = hs[(s + t) % world]
                for r0 in range(0, n, per):
                    nr = min(per, n - r0)
                    base = (shard_ptr if t == 0 else rows_ptr) + r0 * rowb
                    ops.chain_piece_i32(h, nr, nr, first + r0, nr, base, rows_ptr + r0 * rowb, rec_ptr, side.cuda_stream)
                ops.chain_close_i32(h, n, n, first, n, rows_ptr, rec_ptr, t, side.cuda_stream)
            side.synchronize()
            if records is not None:
                records.append((c, s, _rec(buf[:REC])))
            if known_closed:
                # the slice left closed: it must come home as the store holds it, record included
                assert bytes(buf[:REC].cpu().numpy().tobytes()) == bytes(srec[s].cpu().numpy().tobytes())
                assert buf[REC:].cpu().numpy().tobytes() == _values(stores[s]).tobytes()
            else:
                ops.assign_i32(stores[s], rows_ptr, n * cols, rec_ptr)
                srec[s] = buf[:REC].clone()
            keep.append(buf)
            torch.cuda.synchronize()
        for r, h in enumerate(hs):
            try:
                ops.end(h)
            except Exception as e:
                if end_errors is None:
                    raise
                end_errors.append((c, r, type(e).__name__))
    out = []
    for st in stores:
        try:
            st.flush()
        except IllegalStateException as e:
            assert st.error_state() == (e.code, e.key, e.col)
        out.append((st.values(), st.error_state()))
        st.close()
    return out


def _same(got, want):
    for s, ((gv, ge), (wv, we)) in enumerate(zip(got, want)):
        assert ge == we, (s, ge, we)
        assert gv.dtype == wv.dtype and gv.tobytes() == wv.tobytes(), (s, int((gv != wv).sum()))


# (cols, W, kind, pieces)
CLEAN = [(1024, 11, "perm", 1), (512, 1, "asc", 2), (256, 11, "subset", 4), (1000, 11, "subset", 2),
         (520, 11, "perm", 4), (67, 64, "perm", 2), (3, 64, "perm", 1), (1000, 64, "subset", 1), (67, 1, "perm", 4),
         (3, 11, "asc", 4), (1024, 1, "subset", 4)]


@pytest.mark.parametrize("cols,W,kind,pieces", CLEAN)
def test_clean_calls_match_the_ring_order(oracle, cols, W, kind, pieces):
    """Two calls (one at W = 64), rank 0 passing no push in the second: no error, every shard
    byte-equal to the oracle fed the ring order."""
    ncalls = 1 if W == 64 else 2
    calls = E.calls_of(E.WORLD, W, E.ROWS, cols, ncalls, kind, short=lambda r, c: (r, c) == (0, 1))
    init = E.init_counts(E.ROWS, cols)
    recs = []
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init, records=recs)
    assert all(r[0] is None for _, _, r in recs)
    _same(got, E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init))


@pytest.mark.parametrize("step,cols,pieces", [(0, 67, 2), (1, 1000, 1), (2, 256, 4), (1, 3, 2), (2, 1024, 1)])
def test_first_negative_at_each_ring_step(oracle, step, cols, pieces):
    """Cases 1-3 and 8: the owner's own push, a middle rank's, the last rank's. The slice
    closes at that ring step; the ranks after it, and the whole second call, copy it."""
    calls, init = E.case_negative_at(cols, step)
    recs = []
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init, records=recs)
    want = E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init)
    _same(got, want)
    assert want[1][1][0] == E.NEG
    home = {(c, s): r for c, s, r in recs}
    pos, key, col, at = home[(0, 1)]
    assert pos is not None and pos >> 40 == 1 and (key, col, at) == (want[1][1][1], want[1][1][2], step)
    assert home[(1, 1)] == home[(0, 1)] and home[(1, 0)][0] is None and home[(1, 2)][0] is None


@pytest.mark.parametrize("cols,pieces", [(520, 2), (3, 1)])
def test_two_ranks_the_ring_earlier_one_wins(oracle, cols, pieces):
    calls, init = E.case_two_ranks(cols)
    recs = []
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init, records=recs)
    _same(got, E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init))
    assert {s: r[3] for _, s, r in recs if r[0] is not None} == {1: 1}  # closed by rank 2, ring step 1


@pytest.mark.parametrize("cols,pieces", [(1000, 2), (1000, 4), (67, 4), (512, 2), (1024, 4), (3, 4)])
def test_earliest_position_in_the_last_subchunk_rolls_the_earlier_ones_back(oracle, cols, pieces):
    calls, init = E.case_late_subchunk(cols)
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init)
    want = E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init)
    assert want[0][1][0] == E.NEG
    _same(got, want)


@pytest.mark.parametrize("cols,pieces", [(1000, 2), (3, 1), (256, 1)])
def test_dip_below_zero_raised_again_later(oracle, cols, pieces):
    calls, init = E.case_dip(cols)
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init)
    want = E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init)
    assert want[2][1][0] == E.NEG and want[2][0][11, cols - 1] == -1
    _same(got, want)


@pytest.mark.parametrize("cols,pieces", [(67, 1), (1024, 2), (520, 1)])
def test_int_max_plus_one(oracle, cols, pieces):
    calls, init = E.case_int_max(cols)
    got = run_ring(E.WORLD, E.ROWS, cols, pieces, calls, init)
    want = E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init)
    assert want[0][1] == (E.NEG, 3, 0) and want[0][0][3, 0] == -2 ** 31
    _same(got, want)


def _one_step(cols, pushes, record, base_vals, first=0, pieces=2, rows=E.ROWS):
    """One ring step over rows [first, first + len(base_vals)) of a `rows`-row model, out of
    place into a buffer of 0x5A bytes. Returns (out values, record bytes, end error name)."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    ops, fmt = HipOps(), DataDesc(1, 0, E.VT)
    n, rowb = len(base_vals), cols * 4
    dev = [_dev(p) for p in pushes]
    base = _dev(base_vals)
    out = torch.full((n * rowb,), 0x5A, dtype=torch.uint8, device="cuda")
    rec = _dev(np.frombuffer(record, np.uint8))
    torch.cuda.synchronize()
    h = ops.begin(fmt, 0, rows, cols, [d.data_ptr() for d in dev], [d.numel() for d in dev], 0)
    per = (n + pieces - 1) // pieces
    for r0 in range(0, n, per):
        nr = min(per, n - r0)
        ops.chain_piece_i32(h, nr, nr, first + r0, nr, base.data_ptr() + r0 * rowb, out.data_ptr() + r0 * rowb,
                            rec.data_ptr(), 0)
    ops.chain_close_i32(h, n, n, first, n, out.data_ptr(), rec.data_ptr(), 5, 0)
    torch.cuda.synchronize()
    err = None
    try:
        ops.end(h)
    except Exception as e:
        err = type(e).__name__
    return out.cpu().numpy().view(E.I4).reshape(n, cols), bytes(rec.cpu().numpy().tobytes()), err


@pytest.mark.parametrize("cols", [1000, 256, 3])
def test_closed_slice_is_copied_untouched(cols):
    """Case 8: pushes that would move every row, one of them far below zero, meet a closed
    record: the slice is copied bit for bit and the record keeps its verdict."""
    init = E.init_counts(E.ROWS, cols)
    f, l = X.shard_ranges(E.WORLD, E.ROWS)[2]
    pushes = E.pushes(1, 3, E.ROWS, cols, 0)
    pushes[1] = E.poke(pushes[1], cols, f + 9, 0, E.BIG)
    closed = struct.pack("<QqiIQ", (2 << 40) | 1234, 77, 1, 0, 0)
    out, rec, err = _one_step(cols, pushes, closed, init[f:l + 1], first=f)
    assert err is None and rec == closed and out.tobytes() == init[f:l + 1].tobytes()


@pytest.mark.parametrize("cols", [1000, 512, 3])
def test_failed_index_adds_nothing_and_leaves_the_record_open(cols):
    """Case 9: a key outside the matrix in push 1; push 0 alone would drive a counter negative."""
    init = E.init_counts(E.ROWS, cols)
    f, l = X.shard_ranges(E.WORLD, E.ROWS)[0]
    pushes = E.pushes(2, 3, E.ROWS, cols, 0)
    pushes[0] = E.poke(pushes[0], cols, f + 9, 0, E.BIG)
    keys, vals = E.decode(pushes[1], cols)
    keys[len(keys) // 2] = E.ROWS + 3
    pushes[1] = E.encode(keys, vals)
    out, rec, err = _one_step(cols, pushes, OPEN, init[f:l + 1], first=f)
    assert err == "ArrayIndexOutOfBoundsException" and rec == OPEN and out.tobytes() == init[f:l + 1].tobytes()


@pytest.mark.parametrize("cols", [3, 4])
def test_rollback_of_pushes_taken_as_identity(oracle, cols):
    """57 ascending full-range pushes into 270 000 rows: the slot table (rows x 64 x 4 B) is
    beyond 64 MiB, so dml_prereduce_begin checks every key up front and the index writes no
    slots for these pushes; the pieces and the rollback take slot = row. Push 40 drives a
    counter negative at row 1234: the adds after it come back out."""
    rows, W = 270_000, 57
    init = E.init_counts(rows, cols)
    pushes = E.pushes(0, W, rows, cols, 0, "asc")
    pushes[40] = E.poke(pushes[40], cols, 1234, cols - 1, E.BIG)
    o = oracle.OracleStore(1, 0, E.VT, 0, rows - 1, cols)
    o.data[:] = init
    codes = [o.push_many([p]) for p in pushes[:41]]
    assert codes == [0] * 40 + [E.NEG] and o.error() == (E.NEG, 1234, cols - 1)
    out, rec, err = _one_step(cols, pushes, OPEN, init, pieces=4, rows=rows)
    pos, key, col, step = struct.unpack("<QqiI", rec[:24])
    assert err is None and (pos >> 40, key, col, step) == (40, 1234, cols - 1, 5)
    assert out.tobytes() == np.ascontiguousarray(o.data).tobytes()
    o.close()


def test_closing_commit_puts_the_store_into_its_error_state(oracle):
    """The store learns of the verdict when it next retires the commit: flush raises the
    IllegalStateException with the oracle's key and col, the state is sticky, pushes are refused."""
    from distml_amd import DataDesc, DataStore, KeyRange
    from distml_amd.group import HipOps
    from distml_amd.store import IllegalStateException
    cols, rows = 67, 300
    init = E.init_counts(rows, cols)
    st = DataStore(DataDesc(1, 0, E.VT), KeyRange(0, rows - 1), cols, async_push=True)
    st.load_values(init)
    src = _dev(init + 1)
    rec = _dev(np.frombuffer(struct.pack("<QqiIQ", (1 << 40) | 40, 123, 5, 2, 0), np.uint8))
    push = _dev(E.pushes(0, 1, rows, cols, 0)[0])
    torch.cuda.synchronize()
    HipOps().assign_i32(st, src.data_ptr(), rows * cols, rec.data_ptr())
    with pytest.raises(IllegalStateException) as ei:
        st.flush()
    assert (ei.value.code, ei.value.key, ei.value.col) == (E.NEG, 123, 5) == st.error_state()
    with pytest.raises(IllegalStateException):
        st.pushDevice([push.data_ptr()], [push.numel()])
    with pytest.raises(IllegalStateException):
        HipOps().assign_i32(st, src.data_ptr(), rows * cols, rec.data_ptr())
    assert st.values().tobytes() == (init + 1).tobytes()
    st.close()


def test_new_calls_refuse_other_handles_and_stores(oracle):
    from distml_amd import DataDesc, DataStore, KeyRange, _lib
    from distml_amd.group import HipOps
    from distml_amd.store import NativeError
    ops = HipOps()
    rows, cols = 64, 8
    buf = torch.full((rows * cols * 8,), 0x5A, dtype=torch.uint8, device="cuda")
    rec = _dev(np.frombuffer(OPEN, np.uint8))

    def both_refused(h):
        for call in (lambda: ops.chain_piece_i32(h, rows, rows, 0, rows, buf.data_ptr(), buf.data_ptr(), rec.data_ptr(), 0),
                     lambda: ops.chain_close_i32(h, rows, rows, 0, rows, buf.data_ptr(), rec.data_ptr(), 0, 0)):
            with pytest.raises(NativeError) as ei:
                call()
            assert ei.value.code == _lib.DML_E_UNSUPPORTED

    for fmt in (DataDesc(1, 0, 1), DataDesc(1, 0, 1, False, True, True)):
        p = _dev(oracle.synth_dense_bucket(0, fmt.valueType, 0, rows, rows, cols, 3, 1, 0))
        torch.cuda.synchronize()
        h = ops.begin(fmt, 0, rows, cols, [p.data_ptr()], [p.numel()], 0)
        both_refused(h)
        ops.end(h)
    fmt = DataDesc(1, 0, E.VT)
    ctx = ops.ctx_create(fmt, 0, rows, cols, 0)
    p = _dev(oracle.synth_dense_bucket(0, E.VT, 0, rows, rows, cols, 3, 1, 0))
    torch.cuda.synchronize()
    h = ops.begin_ctx(ctx, [p.data_ptr()], [p.numel()], 0)
    both_refused(h)
    ops.end(h)
    ops.ctx_destroy(ctx)
    for fmt in (DataDesc(1, 0, 1), DataDesc(1, 0, 1, False, True, True)):
        st = DataStore(fmt, KeyRange(0, rows - 1), cols, async_push=True)
        before = st.values().tobytes()
        with pytest.raises(NativeError) as ei:
            ops.assign_i32(st, buf.data_ptr(), rows * cols, rec.data_ptr())
        assert ei.value.code == _lib.DML_E_UNSUPPORTED and st.values().tobytes() == before
        st.close()
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all()) and bytes(rec.cpu().numpy().tobytes()) == OPEN

"""GPU, one process: the building blocks of the chained reduce-scatter of AdaGrad
matrices.

dml_prereduce_chain_piece_ada (HipOps.chain_piece_ada): the ring is emulated with one
pre-reduce handle per virtual rank (begun with the AdaGrad descriptor); every shard's
slice — data plane, delta plane, one uint32 mark per row, the maxDelta record — walks
the ranks s, s+1, ..., s-1 in a host loop, `pieces` sub-chunks per step, the last one
applying the step's candidates; the owner's store then commits it
(dml_store_assign_adagrad_device, HipOps.assign_ada). data, delta, alpha and maxDelta
are compared byte for byte (unsigned views) with tests/chain_ada_expect.py, the oracle
fed the ring order, after every call.

Which kernel a case reaches (dml_prereduce_chain_piece_ada's dispatch): ascending
full-range pushes of rows of whole 16-B vectors under 4 KiB are checked key by key
before the first piece and run k_chain_ada_ident, the vector stream through the row
map (1198 x 200, 999 x 200 with a blocked row map whose blocks hold no whole number
of waves' rows, 300 x 256); everything else runs k_chain_ada_rows over the slot table
(permuted 64 / 67 / 300 columns, 3 columns, rows no push lists, failed handles).
"""
import struct

import numpy as np
import pytest

import chain_ada_expect as A
import chain_expect as X

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def _record(md):
    """The device record (DML_MAXDELTA_RECORD_BYTES): value, row, col, pad, no pending candidate."""
    return _dev(np.frombuffer(struct.pack("<fiii", *md, 0) + b"\0" * 16, np.uint8).copy())


class Ring:
    """One AdaGrad DataStore per shard and the host loop of the ring."""

    def __init__(self, world, rows, cols, init):
        from distml_amd import DataDesc, DataStore, KeyRange
        from distml_amd.group import HipOps
        self.ops, self.fmt = HipOps(), DataDesc(1, 0, 1, False, True, True)
        assert self.fmt.adaGrad
        self.world, self.rows, self.cols = world, rows, cols
        self.ranges = X.shard_ranges(world, rows)
        self.stores = []
        for f, l in self.ranges:
            st = DataStore(self.fmt, KeyRange(f, l), cols, async_push=True)
            st.load_values(init[f:l + 1])
            self.stores.append(st)
        self.side = torch.cuda.Stream()
        self.keep = []

    def close(self):
        for st in self.stores:
            st.close()

    def state(self):
        out = []
        for st in self.stores:
            alpha, delta = st.adagrad_state()
            out.append(dict(data=st.values(), delta=delta, alpha=alpha, md=st.maxDelta()))
        return out

    def call(self, per_rank, pieces, blocked=False, inplace=True, end_errors=None, c=0, probe=None):
        """One chained call: a handle per virtual rank (all its pushes, whole model), slice s
        through ranks s, s+1, ..., s-1, then the owner's commit. probe(s, t, before, after):
        sees the travelling planes (host copies) around step t of slice s."""
        ops, world, rows, cols = self.ops, self.world, self.rows, self.cols
        rowb = cols * 4
        dev = [[_dev(p) for p in per_rank[r]] for r in range(world)]
        self.keep.append(dev)
        torch.cuda.synchronize()
        hs = [ops.begin(self.fmt, 0, rows, cols, [d.data_ptr() for d in dev[r]], [d.numel() for d in dev[r]], 0)
              for r in range(world)]
        for s, (first, last) in enumerate(self.ranges):
            n = last - first + 1
            per = (n + pieces - 1) // pieces
            st = self.stores[s]
            alpha, delta = st.adagrad_state()
            cur = [_dev(st.values()), _dev(delta), None, _record(st.maxDelta())]  # marks None: all clear
            del alpha
            for t in range(world):
                h = hs[(s + t) % world]
                out = [cur[0] if inplace else torch.empty_like(cur[0]), cur[1] if inplace else torch.empty_like(cur[1]),
                       cur[2] if inplace and cur[2] is not None else torch.full((n * 4,), 0xAB, dtype=torch.uint8,
                                                                                  device="cuda"), cur[3]]
                before = self._snap(cur) if probe else None
                chunks = [(0, n)] if blocked else [(r0, min(per, n - r0)) for r0 in range(0, n, per)]
                for i, (r0, nr) in enumerate(chunks):
                    bm = 0 if cur[2] is None else cur[2].data_ptr() + r0 * 4
                    ops.chain_piece_ada(h, per if blocked else nr, per if blocked else nr, first + r0, nr,
                                        cur[0].data_ptr() + r0 * rowb, cur[1].data_ptr() + r0 * rowb, bm,
                                        out[0].data_ptr() + r0 * rowb, out[1].data_ptr() + r0 * rowb,
                                        out[2].data_ptr() + r0 * 4, out[3].data_ptr(), i == len(chunks) - 1,
                                        self.side.cuda_stream)
                self.keep.append(cur)
                cur = out
                if probe:
                    self.side.synchronize()
                    probe(s, t, before, self._snap(cur))
            self.side.synchronize()
            ops.assign_ada(st, cur[0].data_ptr(), cur[1].data_ptr(), cur[2].data_ptr(), cur[3].data_ptr())
            self.keep.append(cur)
        for r, h in enumerate(hs):
            try:
                ops.end(h)
            except Exception as e:
                if end_errors is None:
                    raise
                end_errors.append((c, r, type(e).__name__))
        torch.cuda.synchronize()

    @staticmethod
    def _snap(cur):
        return [None if x is None else x.cpu().numpy().copy() for x in cur]


def assert_state(got, want, tag, alpha_skip=None):
    for s, (g, w) in enumerate(zip(got, want)):
        for k in ("data", "delta", "alpha"):
            gb, wb = X.bits(g[k], A.VT), X.bits(w[k], A.VT)
            if k == "alpha" and alpha_skip is not None:
                keep = ~alpha_skip[s]
                assert (gb[keep] == wb[keep]).all(), (tag, s, k, int((gb[keep] != wb[keep]).sum()))
            else:
                assert gb.shape == wb.shape and (gb == wb).all(), (tag, s, k, int((gb != wb).sum()))
        assert A.same_md(g["md"], w["md"]), (tag, s, g["md"], w["md"])


@pytest.mark.parametrize("world,rows,cols,pieces,asc,blocked", A.RING_CASES)
def test_ada_chain_matches_the_ring_order(oracle, world, rows, cols, pieces, asc, blocked):
    """Two calls of W = 5 pushes per rank (past the store kernels' 4-push chunk; call 1: rank 0
    passes none): data, delta, alpha and maxDelta byte-equal to the oracle after each call."""
    calls = A.ring_calls(world, rows, cols, asc)
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init)
    ring = Ring(world, rows, cols, init)
    try:
        for c, per_rank in enumerate(calls):
            ring.call(per_rank, pieces, blocked=blocked)
            assert_state(ring.state(), want[c], (c,))
    finally:
        ring.close()


@pytest.mark.parametrize("cols,asc", [(200, True), (64, False)])
def test_ada_chain_in_place_equals_out_of_place(oracle, cols, asc):
    world, rows = 3, 1198 if asc else 1000
    calls = A.calls(world, 3, rows, cols, 1, asc=asc)
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init)
    states = []
    for inplace in (True, False):
        ring = Ring(world, rows, cols, init)
        try:
            ring.call(calls[0], 2, inplace=inplace)
            states.append(ring.state())
        finally:
            ring.close()
    assert_state(states[0], want[0], "in place")
    assert_state(states[1], want[0], "out of place")


@pytest.mark.parametrize("asc", [False, True])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_ada_chain_max_delta_ties(oracle, case, asc):
    """Exact 4.0 maxima (chain_ada_expect.tie_calls): (a) the earlier ring position holds the
    tie though its element sits in the slice's first piece and the later rank's in the second;
    (b) inside one rank the earlier push holds it though its piece ran second; (c) a maximum
    the store already held stays."""
    calls, holder, _ = A.tie_calls(case, asc)
    init = X.init_values(A.VT, A.TIE_ROWS, A.TIE_COLS)
    want = A.expected(oracle, A.TIE_WORLD, A.TIE_ROWS, A.TIE_COLS, calls, init)
    ring = Ring(A.TIE_WORLD, A.TIE_ROWS, A.TIE_COLS, init)
    try:
        for c, per_rank in enumerate(calls):
            ring.call(per_rank, A.TIE_PIECES)
            got = ring.state()
            assert got[1]["md"] == (4.0, holder[0], holder[1]), (c, got[1]["md"])
            assert_state(got, want[c], (case, c))
    finally:
        ring.close()


def test_ada_chain_set_alpha_and_untouched_rows(oracle):
    """Call 0 lists every row; setAlpha(0.05, 1e-4, 2.0) on stores and oracle; call 1 leaves every
    7th row unlisted and lists one row with zero gradients only. Unlisted rows keep the set
    alpha though their delta is above 1; the zero-gradient row is recomputed."""
    world, W, rows, cols = 2, 5, 300, 64
    calls = A.set_alpha_calls(world, W, rows, cols)
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init, set_alpha={0: A.SET_ALPHA})
    ring = Ring(world, rows, cols, init)
    try:
        ring.call(calls[0], 2)
        for st in ring.stores:
            st.setAlpha(*A.SET_ALPHA)
        assert_state(ring.state(), want[0], 0)
        ring.call(calls[1], 2)
        got = ring.state()
        assert_state(got, want[1], 1)
        un = np.arange(5, rows // world, 7)  # shard 0's unlisted rows
        assert (got[0]["alpha"][un] == np.float32(A.SET_ALPHA[0])).all() and (got[0]["delta"][un] > 1).any()
        z = got[0]["delta"][A.ZERO_ROW] > 1
        assert z.any() and (got[0]["alpha"][A.ZERO_ROW][z] != np.float32(A.SET_ALPHA[0])).all()
    finally:
        ring.close()


def test_ada_chain_special_values(oracle):
    """-0.0 in listed and unlisted init rows, one +Inf gradient (exact everywhere, it holds
    maxDelta), and in call 1 one NaN gradient on each of two elements of different shards: data
    and delta NaN exactly where the oracle's are, alpha byte-equal everywhere but on those two
    elements, which keep the alpha they held before the call (the documented divergence)."""
    world, W, rows, cols = 3, 5, 300, 64
    calls, inf_el, nan_els = A.special_calls(world, W, rows, cols)
    init = X.minus_zero_init(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init)
    ring = Ring(world, rows, cols, init)
    try:
        ring.call(calls[0], 2)
        got0 = ring.state()
        assert_state(got0, want[0], 0)
        ring.call(calls[1], 2)
        got1 = ring.state()
        skip = [A.nan_alpha_mask(w["delta"]) for w in want[1]]
        assert sum(int(m.sum()) for m in skip) == 2
        assert_state(got1, want[1], 1, alpha_skip=skip)
        for s in range(world):
            assert X.same_bits(got1[s]["alpha"][skip[s]], got0[s]["alpha"][skip[s]], A.VT)
            assert (np.isnan(got1[s]["data"]) == np.isnan(want[1][s]["data"])).all()
        neg0 = X.bits(np.array([-0.0]), A.VT)[0]
        un = np.arange(5, rows // world, 7)
        assert (X.bits(got1[0]["data"], A.VT)[un] == neg0).all()
        assert got1[0]["md"][0] == np.inf or got1[1]["md"][0] == np.inf
    finally:
        ring.close()
    del inf_el, nan_els


def test_ada_chain_failed_handles_forward_unchanged(oracle):
    """Call 0: rank 1's push 1 repeats a row; call 1: rank 2's push 0 holds a key outside the
    matrix. That rank's pieces leave both planes, the marks and the record as they came
    (step 0: the shard's planes, clear marks, the store's record), its _end raises as for the
    plain chain, and the shards equal the yardstick with that rank's call skipped."""
    world, W, rows, cols = 3, 3, 240, 64
    calls = A.calls(world, W, rows, cols, 2)

    def rekey(p, i, key):
        rec = p.reshape(-1, 4 + 4 * cols)
        rec[i, :4] = np.frombuffer(struct.pack("<i", key), np.uint8)

    first_key = int(calls[0][1][1].reshape(-1, 4 + 4 * cols)[0, :4].copy().view("<i4")[0])
    rekey(calls[0][1][1], rows // 2, first_key)  # a repeated row
    rekey(calls[1][2][0], rows // 3, rows + 3)   # outside the matrix
    bad = {(1, 0), (2, 1)}
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init, skip=lambda r, c: (r, c) in bad)
    ring = Ring(world, rows, cols, init)
    errs, seen = [], []
    try:
        for c, per_rank in enumerate(calls):
            def probe(s, t, before, after, c=c):
                if ((s + t) % world, c) not in bad:
                    return
                seen.append((c, s, t))
                assert (before[0] == after[0]).all() and (before[1] == after[1]).all(), (c, s, t)
                # the record: value, row, col as they came, and no pending candidate left behind
                assert (before[3][:12] == after[3][:12]).all() and not after[3][20:24].any(), (c, s, t)
                if before[2] is None:
                    assert not after[2].any(), (c, s, t)
                else:
                    assert (before[2] == after[2]).all(), (c, s, t)
            ring.call(per_rank, 2, end_errors=errs, c=c, probe=probe)
            assert_state(ring.state(), want[c], c)
    finally:
        ring.close()
    assert len(seen) == 2 * world
    assert errs == [(0, 1, "NativeError"), (1, 2, "ArrayIndexOutOfBoundsException")], errs


@pytest.mark.parametrize("cols", [67, 64])
def test_store_assign_ada_between_pushes(oracle, cols):
    """dml_store_assign_adagrad_device: push, assign, push; data, delta, alpha and maxDelta equal
    the oracle restarted from the assigned state. 64 columns is a shape whose plain stores
    speculate into a second buffer, 67 is not: the commit lands in the current buffer either way."""
    from distml_amd import DataDesc, DataStore, KeyRange
    from distml_amd.group import HipOps
    rows, params = 500, (0.1, 1e-3, 1.5)
    fmt = DataDesc(1, 0, 1, False, True, True)
    st = DataStore(fmt, KeyRange(0, rows - 1), cols, async_push=True)
    rng = np.random.default_rng(3)
    st.load_values(rng.standard_normal((rows, cols)).astype(np.float32))
    st.setAlpha(*params)
    a, b = (A.pushes(0, 1, rows, cols, c, 2)[0] for c in (0, 1))
    da, db = _dev(a), _dev(b)
    val = rng.standard_normal((rows, cols)).astype(np.float32)
    val[::9] = -0.0
    dl = (rng.random((rows, cols)) * 2).astype(np.float32)
    marks = (np.arange(rows) % 3 != 0).astype(np.uint32)
    fresh = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols, ada_grad=1)
    md0 = fresh.max_delta()
    fresh.close()
    src = [_dev(val), _dev(dl), _dev(marks), _record(md0)]
    torch.cuda.synchronize()
    st.pushDevice([da.data_ptr()], [da.numel()])
    HipOps().assign_ada(st, *[x.data_ptr() for x in src])
    st.pushDevice([db.data_ptr()], [db.numel()])
    st.flush()
    alpha, delta = st.adagrad_state()
    got = dict(data=st.values(), delta=delta, alpha=alpha, md=st.maxDelta())
    st.close()
    # the oracle: push a (its alpha), the assigned planes with alpha recomputed where marked and
    # delta > 1, then push b
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols, ada_grad=1)
    o.set_alpha(*params)
    assert o.push(a.tobytes()) == 0
    alpha_a = np.array(o.alpha, copy=True)
    o.close()
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols, ada_grad=1)
    o.set_alpha(*params)
    o.data[:] = val
    o.delta[:] = dl
    o.alpha[:] = np.where((marks[:, None] != 0) & (dl > 1), A.alpha_formula(dl, *params), alpha_a)
    assert o.push(b.tobytes()) == 0
    want = dict(data=np.array(o.data), delta=np.array(o.delta), alpha=np.array(o.alpha), md=o.max_delta())
    o.close()
    assert_state([got], [want], cols)


def test_ada_chain_piece_refusals(oracle):
    """The AdaGrad piece refuses a plain-fp32 handle, an int32 handle and a speculative
    context's handle with DML_E_UNSUPPORTED."""
    from distml_amd import DataDesc, _lib
    from distml_amd.group import HipOps
    from distml_amd.store import NativeError
    ops = HipOps()
    rows, cols = 64, 8
    buf = torch.zeros(rows * cols * 4 * 2 + rows * 4 + 32, dtype=torch.uint8, device="cuda")
    p0 = buf.data_ptr()
    args = (rows, rows, 0, rows, p0, p0 + rows * cols * 4, 0, p0, p0 + rows * cols * 4, p0 + rows * cols * 8,
            p0 + rows * cols * 8 + rows * 4, True, 0)
    for fmt in (DataDesc(1, 0, 1), DataDesc(1, 0, 0)):
        p = _dev(oracle.synth_dense_bucket(0, fmt.valueType, 0, rows, rows, cols, 3, 1, 0))
        torch.cuda.synchronize()
        h = ops.begin(fmt, 0, rows, cols, [p.data_ptr()], [p.numel()], 0)
        with pytest.raises(NativeError) as ei:
            ops.chain_piece_ada(h, *args)
        assert ei.value.code == _lib.DML_E_UNSUPPORTED
        ops.end(h)
    fmt = DataDesc(1, 0, 1)
    ctx = ops.ctx_create(fmt, 0, rows, cols, 0)
    p = _dev(oracle.synth_dense_bucket(0, 1, 0, rows, rows, cols, 3, 1, 0))
    torch.cuda.synchronize()
    h = ops.begin_ctx(ctx, [p.data_ptr()], [p.numel()], 0)
    with pytest.raises(NativeError) as ei:
        ops.chain_piece_ada(h, *args)
    assert ei.value.code == _lib.DML_E_UNSUPPORTED
    ops.end(h)
    ops.ctx_destroy(ctx)
    assert not buf.any()

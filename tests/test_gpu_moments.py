"""GPU, one process, no process group: the two-moment AdaGrad kernels bit for bit.

dml_prereduce_moments_piece (k_moments_flat) and dml_store_apply_adagrad_moments_device
(k_ada_moments + k_maxdelta_elems) through distml_amd.group.HipOps, every output compared
byte for byte with tests/moments_expect.py: a float32 model of the kernels' stated
arithmetic (one rounding per add in push order; the store's double alpha formula; a strict
rise of delta as the maxDelta candidate, ties to the lowest row-major position).
tests/test_moments_expect.py anchors that model to the oracle on the CPU and checks that the
inputs used here are what they claim to be.

Pieces: every width at which R = min(16, 512 / (cols / 4)) changes, one / three / 64 pushes,
key subsets, one piece over all rows and a 3-way split in two pieces per slice with its two
padding rows, a NaN guard band behind every output, -0.0 / denormal / Inf / NaN gradients,
failed handles (zeros, the error at _end, the slot table clean afterwards), refusals, and
the all-identity branch (a slot table beyond 64 MiB).
Apply: states made by ordinary pushes, a wide shard, a shard whose first key is 1000,
maxDelta ties inside a vector, a block and across blocks, the alpha rules, refusals, the
order among pushes, and the documented setAlpha divergence.
"""
import struct

import numpy as np
import pytest

import moments_expect as M

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 64  # float32 words behind every output
GUARD_BITS = 0x7FC0BEEF
FILL_BITS = 0x40E00000  # 7.0: what an output holds before a piece writes it


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _fmt(ada=True, vt=M.VT):
    from distml_amd import DataDesc
    return DataDesc(1, 0, vt, False, True, ada)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _args(dev):
    return [d.data_ptr() for d in dev], [d.numel() for d in dev]


def _fresh(nwords):
    """An output of nwords float32 no piece leaves as it found it, and its guard band."""
    a = np.full(nwords + GUARD, FILL_BITS, np.uint32)
    a[nwords:] = GUARD_BITS
    return torch.from_numpy(a.view(np.int32)).cuda()


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _split(out, nwords):
    """(body bytes, guard intact) of an output made by _fresh."""
    w = _words(out)
    return w[:nwords].tobytes(), bool((w[nwords:] == GUARD_BITS).all()) and len(w) == nwords + GUARD


def _moments_call(ops, dev, rows, cols, pieces, first, side, fmt=None):
    """begin, one moments piece per row map entry (each into a buffer of its own, on a side
    stream), _end. Returns (outputs, the exception _end raised or None)."""
    from distml_amd import DistMLException
    outs = [_fresh(n * 2 * cols) for (_, _, _, n) in pieces]
    torch.cuda.synchronize()
    ptrs, lens = _args(dev)
    h = ops.begin(fmt or _fmt(), first, rows, cols, ptrs, lens, torch.cuda.current_stream().cuda_stream)
    err = None
    try:
        for (b, s, o, n), out in zip(pieces, outs):
            ops.moments_piece(h, b, s, o, n, out.data_ptr(), side.cuda_stream)
        side.synchronize()
    finally:
        try:
            ops.end(h)
        except DistMLException as e:
            err = e
    torch.cuda.synchronize()
    return outs, err


def _check_pieces(outs, pushes, rows, cols, pieces, first, what):
    for (b, s, o, n), out in zip(pieces, outs):
        want = M.piece_expect(pushes, rows, cols, b, s, o, n, first=first)
        body, guard = _split(out, n * 2 * cols)
        assert guard, (what, "guard band", (b, s, o, n))
        got = np.frombuffer(body, np.uint32).reshape(n, 2 * cols)
        pad = M.padding_tasks((b, s, o, n)) if rows == M.ROWS else []
        assert not got[pad].any(), (what, "padding rows", (b, s, o, n))
        assert body == want.tobytes(), (what, (b, s, o, n))


# ---- pieces ----------------------------------------------------------------------------------
PIECE_CASES = [(c, p) for c in M.WIDTHS for p in M.PUSH_SETS] + [(c, "many64") for c in M.MANY_WIDTHS]


@pytest.mark.parametrize("row_map", list(M.ROW_MAPS))
@pytest.mark.parametrize("cols,push_set", PIECE_CASES)
def test_pieces(cols, push_set, row_map):
    """Σu and Σu² of every task row, byte for byte, padding rows zero, guard band untouched."""
    from distml_amd.group import HipOps
    pushes = M.piece_pushes(cols, push_set)
    dev = [_dev(p) for p in pushes]
    pieces = M.ROW_MAPS[row_map]
    outs, err = _moments_call(HipOps(), dev, M.ROWS, cols, pieces, M.FIRST, torch.cuda.Stream())
    assert err is None
    _check_pieces(outs, pushes, M.ROWS, cols, pieces, M.FIRST, (cols, push_set, row_map))


@pytest.mark.parametrize("row_map", list(M.ROW_MAPS))
def test_pieces_special_values(row_map):
    """A lone -0.0 gives Σu = +0.0; denormals are summed, their squares vanish; one +Inf gives
    Inf in both halves; one NaN keeps its payload in both."""
    from distml_amd.group import HipOps
    cols = M.SPECIAL_COLS
    pushes = M.special_pushes()
    dev = [_dev(p) for p in pushes]
    pieces = M.ROW_MAPS[row_map]
    outs, err = _moments_call(HipOps(), dev, M.ROWS, cols, pieces, M.FIRST, torch.cuda.Stream())
    assert err is None
    _check_pieces(outs, pushes, M.ROWS, cols, pieces, M.FIRST, ("special", row_map))
    if row_map == "whole":
        got = _words(outs[0])[: M.ROWS * 2 * cols].reshape(M.ROWS, 2 * cols)
        r, c = M.SPECIALS["minus_zero"]
        assert got[r, c] == 0  # +0.0, not 0x80000000
        r, c = M.SPECIALS["nan"]
        assert got[r, c] == M.NAN_BITS and got[r, cols + c] == M.NAN_BITS
        r, c = M.SPECIALS["inf"]
        assert got[r, c] == 0x7F800000 and got[r, cols + c] == 0x7F800000
        r, c = M.SPECIALS["denormal"]
        assert got[r, c] == 426 and got[r, cols + c] == 0


# handles open at once in test_slot_table_comes_back_clean: more than any test of this suite
# holds, so every pooled lease that fits the size passes through them
LEASES = 8


@pytest.mark.parametrize("kind", ["oos", "dup", "good"])
def test_slot_table_comes_back_clean(kind):
    """A handle whose index fails (a key outside the matrix; a row listed twice in one push)
    writes zeros in every task row and _end returns that failure's code; after it, and after
    a good permuted moments handle, a plain piece of a new handle on the same lease and size,
    with other permuted key-subset pushes, is byte-exact: the slot table came back clean, or
    was marked for a reset. Leases are handed out first-fit from a pool, so LEASES handles
    are open at once and each one runs the moments call."""
    from distml_amd import ArrayIndexOutOfBoundsException, DistMLException, NativeError
    from distml_amd._lib import DML_E_KEY_OUT_OF_SHARD, DML_E_UNSUPPORTED
    from distml_amd.group import HipOps
    cols, rows, first = 200, M.ROWS, M.FIRST
    ops, side = HipOps(), torch.cuda.Stream()
    pushes = M.piece_pushes(cols, "full3", seed=7) if kind == "good" else M.failed_pushes(kind, cols)
    dev = [_dev(p) for p in pushes]
    ptrs, lens = _args(dev)
    piece = M.ROW_MAPS["whole"][0]
    outs = [_fresh(rows * 2 * cols) for _ in range(LEASES)]
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    hs, errs = [], []
    try:
        for _ in range(LEASES):
            hs.append(ops.begin(_fmt(), first, rows, cols, ptrs, lens, st))
        for h, out in zip(hs, outs):
            ops.moments_piece(h, *piece, out.data_ptr(), side.cuda_stream)
        side.synchronize()
    finally:
        for h in hs:
            try:
                ops.end(h)
                errs.append(None)
            except DistMLException as e:
                errs.append(e)
    torch.cuda.synchronize()
    assert len(errs) == LEASES
    for e in errs:
        if kind == "good":
            assert e is None
        elif kind == "oos":
            assert isinstance(e, ArrayIndexOutOfBoundsException) and e.code == DML_E_KEY_OUT_OF_SHARD
            assert str(e) == "pre-reduce: key outside the matrix"
        else:
            assert isinstance(e, NativeError) and e.code == DML_E_UNSUPPORTED
            assert str(e) == "pre-reduce: a push repeats a row"
    want = M.piece_expect(pushes, rows, cols, *piece, first=first)
    assert want.any() == (kind == "good")
    for out in outs:
        body, guard = _split(out, rows * 2 * cols)
        assert guard and body == want.tobytes()
    # the plain handle: three other permuted key-subset pushes (rows none of them lists read
    # whatever the table holds for them)
    plain, expect = M.plain_pushes(cols, seed=len(kind))
    pdev = [_dev(p) for p in plain]
    out = _fresh(rows * cols)
    torch.cuda.synchronize()
    pp, pl = _args(pdev)
    h = ops.begin(_fmt(ada=False), first, rows, cols, pp, pl, st)
    try:
        ops.piece(h, rows, rows, 0, rows, out.data_ptr(), side.cuda_stream)
        side.synchronize()
    finally:
        ops.end(h)
    body, guard = _split(out, rows * cols)
    assert guard and body == expect.tobytes()


def test_piece_refusals():
    """DML_E_UNSUPPORTED for 6 and 1024 columns, an f64 handle and a begin_ctx handle;
    DML_E_INVALID_ARG for a null output; the output buffer unchanged every time."""
    from distml_amd import NativeError
    from distml_amd._lib import DML_E_INVALID_ARG, DML_E_UNSUPPORTED
    from distml_amd.group import HipOps
    from distml_amd.store import encode_matrix_push
    ops, side = HipOps(), torch.cuda.Stream()
    rows, first = M.ROWS, M.FIRST
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(6)

    def refused(fmt, cols, vt, code, null_out=False, ctx=False):
        keys = first + rng.permutation(rows)
        vals = rng.standard_normal((rows, cols)).astype({1: np.float32, 3: np.float64}[vt])
        dev = [_dev(np.frombuffer(encode_matrix_push(keys, vals, 0, vt), np.uint8))]
        ptrs, lens = _args(dev)
        out = _fresh(rows * 2 * cols * (2 if vt == 3 else 1))
        before = _words(out).tobytes()
        torch.cuda.synchronize()
        x = ops.ctx_create(fmt, first, rows, cols, 0) if ctx else None
        try:
            h = ops.begin_ctx(x, ptrs, lens, st) if ctx else ops.begin(fmt, first, rows, cols, ptrs, lens, st)
            try:
                with pytest.raises(NativeError) as ei:
                    ops.moments_piece(h, rows, rows, 0, rows, 0 if null_out else out.data_ptr(), side.cuda_stream)
                assert ei.value.code == code, (cols, vt, ctx, null_out)
                if ctx:  # the handle is as usable as before the refusal
                    plain = _fresh(rows * cols)
                    ops.piece(h, rows, rows, 0, rows, plain.data_ptr(), side.cuda_stream)
                    ops.verify(h)
            finally:
                ops.end(h)
        finally:
            if ctx:
                ops.ctx_destroy(x)
        torch.cuda.synchronize()
        assert _words(out).tobytes() == before, (cols, vt, ctx, null_out)
        if ctx:
            want = np.zeros((rows, cols), np.float32)
            want[keys - first] = vals
            assert _split(plain, rows * cols) == (want.tobytes(), True)

    refused(_fmt(), 6, 1, DML_E_UNSUPPORTED)
    refused(_fmt(), 1024, 1, DML_E_UNSUPPORTED)
    refused(_fmt(ada=False, vt=3), 8, 3, DML_E_UNSUPPORTED)
    refused(_fmt(ada=False), 8, 1, DML_E_UNSUPPORTED, ctx=True)
    refused(_fmt(), 8, 1, DML_E_INVALID_ARG, null_out=True)


@pytest.mark.parametrize("case", M.IDENT_CASES)
def test_pieces_identity_branch(case):
    """2 200 000 x 4, two full-range pushes: the slot table is beyond 64 MiB, so ascending
    pushes pass a complete key check and the pieces take slot = row (k_moments_flat's all_id
    branch when both are; the mixed one when the second is rotated). One key outside the
    matrix: zeros and the error."""
    from distml_amd import ArrayIndexOutOfBoundsException
    from distml_amd._lib import DML_E_KEY_OUT_OF_SHARD
    from distml_amd.group import HipOps
    rows, cols = M.IDENT_ROWS, M.IDENT_COLS
    pushes = M.ident_pushes(case)
    dev = [_dev(p) for p in pushes]
    piece = (rows, rows, 0, rows)
    outs, err = _moments_call(HipOps(), dev, rows, cols, [piece], 0, torch.cuda.Stream())
    del dev
    if case == "oos":
        assert isinstance(err, ArrayIndexOutOfBoundsException) and err.code == DML_E_KEY_OUT_OF_SHARD
    else:
        assert err is None
    want = M.piece_expect(pushes, rows, cols, *piece)
    assert want.any() == (case != "oos")
    body, guard = _split(outs[0], rows * 2 * cols)
    assert guard
    assert body == want.tobytes()


# ---- apply -------------------------------------------------------------------------------------
def _store(rows, cols, first, ada=M.ADA):
    from distml_amd import DataStore, KeyRange
    st = DataStore(_fmt(), KeyRange(first, first + rows - 1), cols, device=0)
    st.setAlpha(*ada)
    return st


def _state(st):
    """(data, delta, alpha, md) read back from the store."""
    alpha, delta = st.adagrad_state()
    return st.values(), delta, alpha, st.maxDelta()


def _apply(st, src, rows):
    from distml_amd.group import HipOps
    d = _dev(src)
    torch.cuda.synchronize()
    HipOps().apply_moments(st, d.data_ptr(), rows)
    st.flush()
    return d


def _same_state(got, want, what):
    for name, g, w in zip(("data", "delta", "alpha"), got, want):
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, name)
    assert M.md_bytes(got[3]) == M.md_bytes(want[3]), (what, "maxDelta", got[3], want[3])


def _started(rows, cols, first):
    """A store after three ordinary (oracle-exact) pushes: delta, alpha and maxDelta not trivial."""
    rng = np.random.default_rng([rows, cols, 1])
    st = _store(rows, cols, first)
    st.load_values(M.gradients(rng, rows, cols, 0.1))
    st.handlePushBatch(_fmt(), M.start_pushes(rows, cols, first))
    return st


@pytest.mark.parametrize("rows,cols,first", M.APPLY_SHAPES)
def test_apply_on_a_pushed_state(rows, cols, first):
    """data, delta, alpha and maxDelta after one apply equal the model applied to the state
    read back before it: 200 and 4 columns, 1028 (the apply has no width cap), and a shard
    whose first key is 1000 (maxDelta's row is the key)."""
    st = _started(rows, cols, first)
    try:
        before = _state(st)
        assert (before[1] > 1.0).any() and (before[1] <= 1.0).any() and before[3][0] > 0
        src = M.apply_src(rows, cols)
        keep = _apply(st, src, rows)
        want = M.apply_expect(*before, src, M.ADA, first)
        _same_state(_state(st), want, (rows, cols, first))
        assert first <= want[3][1] < first + rows and want[3] != before[3]
        ends_low = want[1] <= 1.0
        assert ends_low.any() and (_state(st)[2][ends_low] == before[2][ends_low]).all()  # delta <= 1 keeps alpha
        del keep
    finally:
        st.close()


@pytest.mark.parametrize("case", list(M.TIES))
def test_apply_maxdelta_ties(case):
    """Equal maxima in one 16-B vector, in two threads of one block, and in two blocks (the
    later position in block 0's second trip, the earlier in block 5): the lowest row-major
    position holds maxDelta."""
    rows, cols, at, winner = M.TIES[case]
    st = _store(rows, cols, 0)
    try:
        before = _state(st)
        assert not before[1].any()
        src = M.tie_src(case)
        keep = _apply(st, src, rows)
        want = M.apply_expect(*before, src, M.ADA, 0)
        got = _state(st)
        assert got[3] == (4.0, winner[0], winner[1]), got[3]
        _same_state(got, want, case)
        del keep
    finally:
        st.close()


def test_apply_equal_rise_leaves_maxdelta_alone():
    """A best rise equal to the running maxDelta leaves value, row and col alone."""
    rows, cols, first = 157, 8, 30
    st = _store(rows, cols, first)
    try:
        state = _state(st)
        for elems, md in (([((5, 1), 4.0)], (4.0, first + 5, 1)), ([((2, 0), 4.0), ((9, 3), 1.0)], (4.0, first + 5, 1))):
            src = M.single(rows, cols, elems)
            keep = _apply(st, src, rows)
            state = M.apply_expect(*state, src, M.ADA, first)
            got = _state(st)
            assert got[3] == md, got[3]
            _same_state(got, state, elems)
            del keep
    finally:
        st.close()


def test_apply_no_rise_is_no_candidate():
    """An element with Σu² = 0 is no candidate though it holds the largest delta: the state
    (delta 4.0 there, a running maxDelta of 0.5) is assigned as a chained commit would."""
    from distml_amd.group import HipOps
    rows, cols, first = 157, 8, 30
    A, B = (40, 2), (90, 7)
    st = _store(rows, cols, first)
    try:
        delta = np.full((rows, cols), 0.25, np.float32)
        delta[A] = 4.0
        parts = [_dev(np.zeros((rows, cols), np.float32)), _dev(delta), _dev(np.zeros(rows, np.uint32)),
                 _dev(np.frombuffer(struct.pack("<fiii", 0.5, first + 3, 2, 0) + b"\0" * 16, np.uint8))]
        torch.cuda.synchronize()
        HipOps().assign_ada(st, *[p.data_ptr() for p in parts])
        before = _state(st)
        assert before[3] == (0.5, first + 3, 2) and before[1][A] == 4.0
        src = M.single(rows, cols, [(B, 1.0)])
        keep = _apply(st, src, rows)
        got = _state(st)
        assert got[3] == (1.25, first + B[0], B[1]), got[3]
        _same_state(got, M.apply_expect(*before, src, M.ADA, first), "no rise")
        del keep, parts
    finally:
        st.close()


def test_apply_alpha_rules():
    """Elements ending at delta <= 1 keep their alpha; a NaN delta keeps it too (and is no
    maxDelta candidate); an Inf delta gives minAlpha (and holds maxDelta)."""
    rows, cols, first = 157, 200, 0
    st = _started(rows, cols, first)
    try:
        before = _state(st)
        hot = np.argwhere(before[1] > 1.0)
        e_nan, e_inf = tuple(hot[len(hot) // 3]), tuple(hot[2 * len(hot) // 3])
        assert before[2][e_nan] != np.float32(M.ADA[0])  # a computed alpha, not the initial one
        src = M.apply_src(rows, cols, seed=1)
        src.view(np.uint32)[e_nan[0], cols + e_nan[1]] = M.NAN_BITS
        src[e_inf[0], cols + e_inf[1]] = np.inf
        keep = _apply(st, src, rows)
        got = _state(st)
        _same_state(got, M.apply_expect(*before, src, M.ADA, first), "alpha rules")
        assert got[1].view(np.uint32)[e_nan] == M.NAN_BITS and got[2][e_nan] == before[2][e_nan]
        assert np.isposinf(got[1][e_inf]) and got[2][e_inf] == np.float32(M.ADA[1])
        assert got[3] == (np.inf, first + e_inf[0], e_inf[1])
        low = got[1] <= 1.0
        assert low.any() and (got[2][low] == before[2][low]).all()
        del keep
    finally:
        st.close()


def test_apply_refusals():
    """A plain f32 store and 6 columns: DML_E_UNSUPPORTED; rows != the shard's and a null src:
    DML_E_INVALID_ARG. The store is unchanged."""
    from distml_amd import DataStore, KeyRange, NativeError
    from distml_amd._lib import DML_E_INVALID_ARG, DML_E_UNSUPPORTED
    from distml_amd.group import HipOps
    ops = HipOps()
    rows = 37

    def refused(st, cols, nrows, code, null=False):
        src = _dev(np.ones((rows, 2 * cols), np.float32))
        torch.cuda.synchronize()
        before = st.values()
        with pytest.raises(NativeError) as ei:
            ops.apply_moments(st, 0 if null else src.data_ptr(), nrows)
        assert ei.value.code == code, (cols, nrows, null)
        assert st.values().tobytes() == before.tobytes()

    plain = DataStore(_fmt(ada=False), KeyRange(0, rows - 1), 8, device=0)
    ada8, ada6 = _store(rows, 8, 0), _store(rows, 6, 0)
    try:
        refused(plain, 8, rows, DML_E_UNSUPPORTED)
        refused(ada8, 8, rows - 1, DML_E_INVALID_ARG)
        refused(ada6, 6, rows, DML_E_UNSUPPORTED)
        refused(ada8, 8, rows, DML_E_INVALID_ARG, null=True)
        assert not ada8.adagrad_state()[1].any() and not ada6.adagrad_state()[1].any()
    finally:
        for s in (plain, ada8, ada6):
            s.close()


def test_apply_between_pushes(oracle):
    """A push, an apply, a push, no flush between: the store ends as the oracle's first push,
    the model's apply on the oracle's arrays, the oracle's second push. data, delta and alpha
    byte for byte; maxDelta's value (the oracle's own record does not see the apply)."""
    from distml_amd.group import HipOps
    rows, cols, first = 157, 200, 50
    rng = np.random.default_rng(77)
    ps = [bytes(M.encode(first + rng.permutation(rows)[:n], M.gradients(rng, n, cols, 0.7))) for n in (rows, 120)]
    src = M.apply_src(rows, cols, seed=2)
    init = M.gradients(rng, rows, cols, 0.1)
    st = _store(rows, cols, first)
    o = oracle.OracleStore(1, 0, M.VT, first, first + rows - 1, cols, ada_grad=1)
    try:
        st.load_values(init)
        dev = [_dev(np.frombuffer(p, np.uint8)) for p in ps]
        dsrc = _dev(src)
        torch.cuda.synchronize()
        st.pushDevice([dev[0].data_ptr()], [dev[0].numel()])
        HipOps().apply_moments(st, dsrc.data_ptr(), rows)
        st.pushDevice([dev[1].data_ptr()], [dev[1].numel()])
        st.flush()
        got = _state(st)
        o.set_alpha(*M.ADA)
        o.data[:] = init
        assert o.push(ps[0]) == 0
        mid = M.apply_expect(np.array(o.data), np.array(o.delta), np.array(o.alpha), o.max_delta(), src, M.ADA, first)
        o.data[:], o.delta[:], o.alpha[:] = mid[0], mid[1], mid[2]
        assert o.push(ps[1]) == 0
        for name, g, w in zip(("data", "delta", "alpha"), got, (o.data, o.delta, o.alpha)):
            assert g.tobytes() == np.ascontiguousarray(w).tobytes(), name
        assert np.float32(got[3][0]) == np.float32(max(mid[3][0], o.max_delta()[0]))
        assert got[1][got[3][1] - first, got[3][2]] == np.float32(got[3][0])
    finally:
        o.close()
        st.close()


def test_set_alpha_divergence_is_as_documented(oracle):
    """The third known divergence of the two-moment path (include/distml_ps.h):
    after setAlpha, an apply rewrites alpha = f(delta) on every element whose delta is above
    1, also on rows its update does not list, where the reference keeps the new initialAlpha;
    and an unlisted row's -0.0 data becomes +0.0. Pinned here, with the oracle's other
    answer beside it, so the text cannot go stale."""
    rows, cols, first = 157, 8, 0
    st = _started(rows, cols, first)
    o = oracle.OracleStore(1, 0, M.VT, first, first + rows - 1, cols, ada_grad=1)
    try:
        push, src, listed = M.set_alpha_push(rows, cols, first)
        un = np.setdiff1d(np.arange(rows), listed)
        st.setAlpha(*M.NEW_ALPHA)
        data = st.values()
        data[un[0], 0] = -0.0
        st.load_values(data)
        before = _state(st)
        assert (before[2] == np.float32(M.NEW_ALPHA[0])).all() and (before[1][un] > 1.0).any()
        keep = _apply(st, src, rows)
        got = _state(st)
        _same_state(got, M.apply_expect(*before, src, M.NEW_ALPHA, first), "setAlpha")
        above = got[1] > 1.0
        assert (got[2][above] == M.alpha_of(got[1], M.NEW_ALPHA)[above]).all()
        assert (got[2][~above] == np.float32(M.NEW_ALPHA[0])).all()
        # the reference: the same state, setAlpha, the same update as one push
        o.data[:], o.delta[:], o.alpha[:] = before[0], before[1], before[2]
        o.set_alpha(*M.NEW_ALPHA)
        assert o.push(push) == 0
        assert got[1].tobytes() == np.ascontiguousarray(o.delta).tobytes()
        assert got[2][listed].tobytes() == np.ascontiguousarray(o.alpha[listed]).tobytes()
        hot = got[1][un] > 1.0
        assert (o.alpha[un] == np.float32(M.NEW_ALPHA[0])).all()
        assert hot.any() and (got[2][un][hot] != o.alpha[un][hot]).all()
        # -0.0 + (+0.0) = +0.0; the reference never touches the row
        assert np.signbit(o.data[un[0], 0]) and got[0][un[0], 0] == 0 and not np.signbit(got[0][un[0], 0])
        same = np.ones((rows, cols), bool)
        same[un[0], 0] = False
        assert (got[0].view(np.uint32)[same] == np.array(o.data).view(np.uint32)[same]).all()
        del keep
    finally:
        o.close()
        st.close()

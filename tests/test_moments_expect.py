"""CPU: the two-moment yardstick (tests/moments_expect.py) is anchored to the oracle, and the
inputs of tests/test_gpu_moments.py are what they claim to be.

  - with one push per call (no repeated row, no -0.0) the model ends byte-equal to one
    OracleStore in data, delta, alpha and maxDelta (value, row, col);
  - with the world-1 test's kind of inputs (test_adagrad_moments_world1: several pushes per
    call) the model stays inside kat.moments_within, the bound the path promises;
  - the special-value pushes never hand an element two NaNs or create one; the tie inputs
    really tie and name the lowest position; the identity shape really is beyond the 64 MiB
    slot-table threshold; the widths give the rows-per-wave they are listed for; the split
    row map has exactly its two padding rows.
"""
import numpy as np
import pytest

import kat
import moments_expect as M


def _oracle_store(oracle, rows, cols, first, ada=M.ADA):
    o = oracle.OracleStore(1, 0, M.VT, first, first + rows - 1, cols, ada_grad=1)
    o.set_alpha(*ada)
    return o


def _same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_model_equals_oracle_one_push_per_call(oracle):
    rows, cols, first = 157, 12, 40
    rng = np.random.default_rng(12)
    o = _oracle_store(oracle, rows, cols, first)
    init = M.gradients(rng, rows, cols, 0.1)
    o.data[:] = init
    state = (init.copy(), np.array(o.delta), np.array(o.alpha), o.max_delta())
    for _ in range(4):
        order = rng.permutation(rows)[:100]
        g = M.gradients(rng, 100, cols, 0.6)
        assert not (np.signbit(g) & (g == 0)).any()
        p = M.encode(first + order, g)
        assert o.push(p) == 0
        src = M.piece_expect([p], rows, cols, rows, rows, 0, rows, first=first)
        state = M.apply_expect(*state, src, M.ADA, first)
        assert _same(state[0], o.data) and _same(state[1], o.delta) and _same(state[2], o.alpha)
        assert M.md_bytes(state[3]) == M.md_bytes(o.max_delta())
    assert 0.2 <= float((o.delta > 1.0).mean()) <= 0.8  # alpha both moved and stayed
    o.close()


def test_model_within_the_path_bound(oracle):
    """3 calls x 4 pushes (ascending, two permuted, a permuted half) at 157 x 12, no flush."""
    rows, cols, calls, W = 157, 12, 3, 4
    rng = np.random.default_rng(44)
    host = []
    for c in range(calls):
        for b in range(W):
            keys = np.arange(rows) if b == 0 else rng.permutation(rows)[: rows if b < 3 else rows // 2]
            host.append(bytes(M.encode(keys, M.gradients(rng, len(keys), cols, 0.6))))
    init = (np.random.default_rng(3).standard_normal((rows, cols)) * 0.1).astype(np.float32)
    o = _oracle_store(oracle, rows, cols, 0, (0.025, 0.0001, 1.5))
    o.data[:] = init
    state = (init.copy(), np.array(o.delta), np.array(o.alpha), o.max_delta())
    for c in range(calls):
        src = M.piece_expect(host[c * W:(c + 1) * W], rows, cols, rows, rows, 0, rows)
        state = M.apply_expect(*state, src, (0.025, 0.0001, 1.5), 0)
    for h in host:
        assert o.push(h) == 0
    kat.moments_within(state[0], state[2].astype(np.float64), state[1].astype(np.float64), o, init, host, cols, "model")
    ov = o.max_delta()[0]
    mv, mr, mc = state[3]
    assert abs(mv - ov) <= 1e-6 * ov and state[1][mr, mc] == np.float32(mv)
    o.close()


def test_piece_model_edges():
    cols = 4
    a = M.encode(M.FIRST + np.array([2, 0]), np.array([[1, 2, 3, 4], [-0.0, 0.5, 0, 1e-30]], np.float32))
    b = M.encode(M.FIRST + np.array([2]), np.array([[1e8, -2, 0.25, 4]], np.float32))
    out = M.piece_expect([a, b], 3, cols, 2, 2, 0, 4, first=M.FIRST)  # task rows 0, 1, 2, 3 (padding)
    want = np.zeros((4, 8), np.float32)
    want[0] = [0.0, 0.5, 0, 1e-30, 0, 0.25, 0, 0]
    want[2] = [np.float32(1) + np.float32(1e8), 0, 3.25, 8, np.float32(1) + np.float32(1e16), 8, 9.0625, 32]
    assert _same(out, want)  # the lone -0.0 came out +0.0; row 1 unlisted; row 3 padding
    for bad in (M.encode(M.FIRST + np.array([0, 3]), np.ones((2, cols), np.float32)),
                M.encode(M.FIRST + np.array([1, 1]), np.ones((2, cols), np.float32))):
        assert not M.piece_expect([a, bad], 3, cols, 3, 3, 0, 3, first=M.FIRST).any()


def test_widths_give_their_rows_per_wave():
    assert [M.rows_per_wave(c) for c in M.WIDTHS] == [16, 16, 16, 15, 10, 3, 2, 2]
    assert 1020 // 4 * 2 == 510 and 128 // 4 * 16 == 512  # vectors per wave of the last and the exact width
    assert all(c % 4 == 0 and c * 4 < 4096 for c in M.WIDTHS)


def test_row_maps_cover_every_row_once():
    for name, pieces in M.ROW_MAPS.items():
        seen = []
        for (b, s, o, n) in pieces:
            t = np.arange(n)
            seen.append((t // b) * s + o + t % b)
        seen = np.sort(np.concatenate(seen))
        assert np.array_equal(seen[seen < M.ROWS], np.arange(M.ROWS)), name
    assert [len(M.padding_tasks(p)) for p in M.ROW_MAPS["split3"]] == [0, 2]
    assert not len(M.padding_tasks(M.ROW_MAPS["whole"][0]))


@pytest.mark.parametrize("push_set", M.PUSH_SETS + ["many64"])
def test_push_sets_are_as_named(push_set):
    cols = 4
    ps = M.piece_pushes(cols, push_set)
    assert len(ps) == {"one": 1, "full3": 3, "subset3": 3, "many64": 64}[push_set]
    listed = np.zeros(M.ROWS, bool)
    for p in ps:
        keys, _ = M.decode(p, cols)
        assert len(np.unique(keys)) == len(keys) and keys.min() >= M.FIRST and keys.max() < M.FIRST + M.ROWS
        listed[keys - M.FIRST] = True
    _, _, ok = M.sums(ps, M.ROWS, cols, M.FIRST)
    assert ok
    if push_set == "subset3":
        assert not listed[M.UNLISTED].any() and listed.sum() < M.ROWS - len(M.UNLISTED) + 1
        assert all(len(M.decode(p, cols)[0]) < M.ROWS for p in ps)
    else:
        assert listed.all()
    if push_set in ("full3", "many64"):
        k0, k1 = M.decode(ps[0], cols)[0], M.decode(ps[1], cols)[0]
        assert np.array_equal(k0, M.FIRST + np.arange(M.ROWS)) and not np.array_equal(k1, k0)


def test_special_inputs_follow_the_nan_rule():
    cols = M.SPECIAL_COLS
    ps = M.special_pushes()
    assert M.special_rule_holds(ps, M.ROWS, cols)
    su, s2, ok = M.sums(ps, M.ROWS, cols, M.FIRST)
    assert ok
    # exactly one NaN element, with the payload, and one Inf element, in both halves
    r, c = M.SPECIALS["nan"]
    assert int(np.isnan(su).sum()) == 1 and int(np.isnan(s2).sum()) == 1
    assert su.view(np.uint32)[r, c] == M.NAN_BITS and s2.view(np.uint32)[r, c] == M.NAN_BITS
    r, c = M.SPECIALS["inf"]
    assert int(np.isinf(su).sum()) == 1 and np.isposinf(su[r, c]) and np.isposinf(s2[r, c])
    r, c = M.SPECIALS["minus_zero"]
    listing = [b for b, p in enumerate(ps) if (M.decode(p, cols)[0] == M.FIRST + r).any()]
    assert listing == [1]
    k, g = M.decode(ps[1], cols)
    assert np.signbit(g[k == M.FIRST + r][0, c]) and not np.signbit(su[r, c]) and su[r, c] == 0
    r, c = M.SPECIALS["denormal"]
    tiny = np.finfo(np.float32).smallest_subnormal
    assert su[r, c] == tiny * np.float32(426) and s2[r, c] == 0 and not np.signbit(s2[r, c])
    r, c = M.SPECIALS["mixed_denormal"]
    assert su[r, c] != 0 and 0 < abs(su[r, c]) < 1
    # a rule breaker is seen
    bad = M.encode([M.FIRST + 120], np.full((1, cols), np.nan, np.float32))
    assert not M.special_rule_holds(ps + [bad], M.ROWS, cols)


@pytest.mark.parametrize("kind", ["oos", "dup"])
def test_failed_inputs_fail(oracle, kind):
    cols = 8
    ps = M.failed_pushes(kind, cols)
    assert not M.sums(ps, M.ROWS, cols, M.FIRST)[2]
    assert M.sums([ps[0], ps[2]], M.ROWS, cols, M.FIRST)[2]  # push 1 alone is the bad one
    o = _oracle_store(oracle, M.ROWS, cols, M.FIRST)
    assert o.push(ps[0]) == 0
    assert (o.push(ps[1]) != 0) == (kind == "oos")  # a repeated row is no error of the reference
    o.close()


def test_tie_inputs_tie():
    for case, (rows, cols, at, winner) in M.TIES.items():
        src = M.tie_src(case)
        sq = src[:, cols:]
        top = sq.max()
        assert top == M.TIE_VALUE and sorted(zip(*np.nonzero(sq == top))) == sorted(at), case
        assert winner == min(at), case
        z = np.zeros((rows, cols), np.float32)
        md = M.apply_expect(z, z, z, (0.0, 0, 0), src, M.ADA, 0)[3]
        assert md == (4.0, winner[0], winner[1]), case
    rows, cols, at, _ = M.TIES["vector"]
    assert at[0][0] == at[1][0] and at[0][1] // 4 == at[1][1] // 4
    rows, cols, at, _ = M.TIES["block"]
    vec = [(r * cols + c) // 4 for r, c in at]
    assert vec[0] != vec[1] and max(vec) < 256
    rows, cols, at, _ = M.TIES["blocks"]
    vec = [(r * cols + c) // 4 for r, c in at]
    blocks = [(v // 256) % M.K_MOMENT_BLOCKS for v in vec]
    trips = [v // (256 * M.K_MOMENT_BLOCKS) for v in vec]
    assert blocks == [0, 5] and trips == [1, 0] and max(vec) < rows * cols // 4


def test_apply_model_candidate_rules():
    cols = 4
    z = np.zeros((3, cols), np.float32)
    delta = z.copy()
    delta[2, 1] = 9.0  # the largest delta, no rise
    src = M.single(3, cols, [((0, 3), 4.0), ((1, 0), 4.0)])
    # a best rise equal to the running value leaves the record alone
    assert M.apply_expect(z, delta, z, (4.0, 77, 1), src, M.ADA, 10)[3] == (4.0, 77, 1)
    # strictly above: the lowest position of the equal maxima, as a key; (2, 1) is no candidate
    assert M.apply_expect(z, delta, z, (3.5, 77, 1), src, M.ADA, 10)[3] == (4.0, 10, 3)
    # NaN keeps alpha and is no candidate; Inf gives minAlpha and is one
    alpha = np.full((3, cols), 0.5, np.float32)
    src = M.single(3, cols, [((0, 0), np.nan), ((1, 1), np.inf), ((2, 2), 0.5), ((2, 3), 4.0)])
    _, nd, na, md = M.apply_expect(z, z, alpha, (0.0, 0, 0), src, M.ADA, 0)
    assert np.isnan(nd[0, 0]) and na[0, 0] == np.float32(0.5)
    assert na[1, 1] == np.float32(M.ADA[1]) and md == (np.inf, 1, 1)
    assert na[2, 2] == np.float32(0.5)  # ends at 0.5 <= 1
    assert na[2, 3] == np.float32(np.float64(np.float32(0.025)) / (np.float64(np.float32(1.5)) * 2.0))


def test_identity_shape_is_beyond_the_threshold():
    assert M.ident_table_bytes() > M.IDENT_MIN_BYTES
    # and not by much: a tenth fewer rows would stay below it
    assert M.ident_table_bytes(M.IDENT_ROWS * 9 // 10) < M.IDENT_MIN_BYTES
    ps = M.ident_pushes("mixed")
    k0, k1 = (M.decode(p, M.IDENT_COLS)[0] for p in ps)
    asc = np.arange(M.IDENT_ROWS)
    assert np.array_equal(k0, asc) and np.array_equal(k1, np.roll(asc, 1))
    del ps, k0, k1
    bad = M.decode(M.ident_pushes("oos")[1], M.IDENT_COLS)[0]
    assert int((bad >= M.IDENT_ROWS).sum()) == 1 and len(bad) == M.IDENT_ROWS


@pytest.mark.parametrize("rows,cols,first", M.APPLY_SHAPES)
def test_apply_inputs_move_and_keep_alpha(oracle, rows, cols, first):
    o = _oracle_store(oracle, rows, cols, first)
    for p in M.start_pushes(rows, cols, first):
        assert o.push(p) == 0
    before = (np.array(o.data), np.array(o.delta), np.array(o.alpha), o.max_delta())
    assert 0.2 <= float((before[1] > 1.0).mean()) <= 0.8
    src = M.apply_src(rows, cols)
    assert not src[M.ZERO_ROWS].any() and np.signbit(src[M.ZERO_ROWS.start, 0])
    data, nd, alpha, md = M.apply_expect(*before, src, M.ADA, first)
    crossed = (before[1] <= 1.0) & (nd > 1.0)
    assert crossed.any() and (nd <= 1.0).any() and (nd == before[1]).any()
    assert (alpha[nd <= 1.0] == before[2][nd <= 1.0]).all()
    assert md[0] > before[3][0] and first <= md[1] < first + rows  # the record moves, its row is a key
    o.close()


def test_set_alpha_case_differs_from_the_oracle(oracle):
    """The documented divergence: after setAlpha, rows an update does not list keep the new
    initialAlpha in the reference; the two-moment apply rewrites alpha = f(delta) wherever
    delta is above 1."""
    rows, cols, first = 157, 8, 0
    o = _oracle_store(oracle, rows, cols, first)
    for p in M.start_pushes(rows, cols, first):
        assert o.push(p) == 0
    o.set_alpha(*M.NEW_ALPHA)
    before = (np.array(o.data), np.array(o.delta), np.array(o.alpha), o.max_delta())
    push, src, listed = M.set_alpha_push(rows, cols, first)
    assert o.push(push) == 0
    _, nd, alpha, _ = M.apply_expect(*before, src, M.NEW_ALPHA, first)
    assert _same(nd, o.delta)
    assert _same(alpha[listed], o.alpha[listed])
    un = np.setdiff1d(np.arange(rows), listed)
    hot = nd[un] > 1.0
    assert hot.any() and (alpha[un][hot] != o.alpha[un][hot]).all()
    assert (o.alpha[un] == np.float32(M.NEW_ALPHA[0])).all()
    assert _same(alpha[un][~hot], o.alpha[un][~hot])
    o.close()


def test_bindings_exist():
    from distml_amd import _lib
    from distml_amd.group import HipOps
    assert "dml_prereduce_moments_piece" in _lib.SIGNATURES
    assert "dml_store_apply_adagrad_moments_device" in _lib.SIGNATURES
    assert hasattr(HipOps, "moments_piece") and hasattr(HipOps, "apply_moments")

"""Device pushes where the product puts them: packed back to back at 4-byte-aligned
addresses (tests/geom.py), with poisoned guard bands, and with keys whose high word
is not zero.

Every other GPU test hands each push to the store in its own 256-byte-aligned
allocation. Here the pushes of a call lie in one arena, the first at an address that
is 0, 4, 8 or 12 mod 16, each next one wherever the record strides put it, and the
bytes around them are a poison word that is NaN as f32 and f64, huge as an int32
counter and outside the shard as a key. A wrong span, tail shift or record offset
reads a neighbour's record or the poison and changes the compared bytes; a stray store
changes the arena, which is compared byte for byte after the run. Comparisons are
bytes-equal against the CPU oracle, as in tests/test_gpu_parity.py, and every case
asserts the kernel instantiation that ran.

Limits: the tests work by values and guard bytes only. No push is placed against the
end of a mapping and nothing here tries to make an out-of-range read fault, so an
over-read whose result is discarded is not seen.

The sparse big-leaf path (k_sp_leaf_big) runs at all four leads, at the smallest shard
that reaches it (11.5 M records, test_sparse_big_leaf_packed).
"""
import numpy as np
import pytest

import geom
import kat
import sparse_route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


_REF = {}


def reference(case, oracle):
    """The oracle's result for a case, computed once and shared by its leads."""
    if case["id"] not in _REF:
        init, pushes, o, rc = geom.oracle_run(case, oracle)
        assert rc == 0
        ref = dict(init=init, pushes=pushes, data=o.data.copy())
        if case["ada"]:
            ref.update(alpha=o.alpha.copy(), delta=o.delta.copy(), max_delta=o.max_delta())
        _REF[case["id"]] = ref
    return _REF[case["id"]]


def run_case(oracle, case, lead, separated=False):
    from distml_amd import DataDesc, DataStore, KeyRange
    ref = reference(case, oracle)
    fmt = DataDesc(case["dt"], case["kt"], case["vt"], False, True, case["ada"])
    s = DataStore(fmt, KeyRange(case["first"], case["first"] + case["rows"] - 1), case["cols"])
    try:
        if case["knob"]:
            s.set_knob(1, 0)  # DML_KNOB_IDENT_FULL_MIN_BYTES: k_ada_ident at this size
        if case["ada"]:
            s.setAlpha(*geom.ADA)
        s.load_values(ref["init"])
        a = geom.pack(ref["pushes"], lead, separated)
        assert all(p % 16 == (lead + o - a.offs[0]) % 16 for p, o in zip(a.ptrs, a.offs))
        n, calls = case["n"], case["calls"]
        cuts = [n * c // calls for c in range(calls + 1)]
        s.stats(reset=True)
        for c0, c1 in zip(cuts, cuts[1:]):
            s.pushDevice(a.ptrs[c0:c1], a.lens[c0:c1])
        s.flush()
        assert s.error_state()[0] == 0
        name = s.kernel_name()
        got = s.values()
        assert kat.bits_equal(got, ref["data"]), (case["id"], lead, name, _first_diff(got, ref["data"]))
        if case["ada"]:
            al, de = s.adagrad_state()
            assert kat.bits_equal(al, ref["alpha"]) and kat.bits_equal(de, ref["delta"]), (case["id"], lead, name)
            assert s.maxDelta() == ref["max_delta"], (case["id"], lead, name)
        if case["want"]:
            geom.kernel_is(name, case["want"][0], **case["want"][1])
        if case.get("spec"):
            st = s.stats()
            assert st["chunks"] == calls and st["spec_chunks"] == case["spec"], st
        if case["kind"] == "sparse":
            # the route tests/sparse_route.py derives from the same bytes: single pass; the fp32
            # cases' repeated key sends one leaf through the compact replay (branch 2)
            if "route" not in ref:
                ref["route"] = sparse_route.call_routes(case["vt"], case["kt"], case["first"], case["rows"],
                                                        ref["pushes"])
            want, kname = sparse_route.expect(ref["route"])
            st = s.stats()
            assert {k: st[k] for k in want} == want and name == kname, (st, want, name, kname)
            assert want == dict(sparse_big_chunks=0, sparse_counted_chunks=0, sparse_replays=int(case["vt"] == 1))
        a.check()
    finally:
        s.close()


def _first_diff(got, want):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1))
    if not len(bad):
        return None
    r, c = int(bad[0][0]), int(bad[0][1]) // g.itemsize
    return dict(rows_differing=int(len(np.unique(bad[:, 0]))), row=r, col=c, got=g[r, c].item(), want=w[r, c].item())


@pytest.mark.parametrize("lead", geom.LEADS)
@pytest.mark.parametrize("case", geom.MATRIX_CASES, ids=lambda c: c["id"])
def test_packed_matrix_pushes(oracle, case, lead):
    """Every dense kernel family on packed pushes, at the four alignments of the first
    push: k_reduce (generic and AdaGrad), k_reduce_rows FULL (CPW 4 / 2 / 1) and DEPTH
    3 (ragged rows, two waves per row), k_reduce_flat, k_flat_ident (1, 3, 9 pushes),
    speculative chunks over two calls, k_ada_flat and k_ada_ident. Row counts 301 and
    1 237: no rows-per-wave divides them."""
    run_case(oracle, case, lead)


@pytest.mark.parametrize("lead", geom.LEADS)
@pytest.mark.parametrize("case", geom.KEY_CASES, ids=lambda c: c["id"])
def test_key_geometry(oracle, case, lead):
    """Keys whose high word matters: shards that start at 2^33 + 7, that straddle 2^31,
    or (int32 keys) that start below zero, through the index, the identity checks and
    the reduces' verifying loops; `alias` cases add 2^32 to three keys of one push, at
    records the identity sample does not see: the reference's (int)(key - first) lands
    on the same row, so the store must update it, whether the chunk stays speculative
    or re-runs (only the result and the error state are asserted). AdaGrad cases with
    int64 keys above 2^31 compare maxDelta's row with the oracle's (int)key."""
    run_case(oracle, case, lead)


@pytest.mark.parametrize("lead", geom.LEADS)
@pytest.mark.parametrize("case", geom.SPARSE_CASES, ids=lambda c: c["id"])
def test_packed_sparse_pushes(oracle, case, lead):
    """Sparse arrays through pushDevice: 8-, 12- and 16-byte records (so pushes start
    at every multiple of 4), 4 pushes of 5 000 keys into 50 000 rows, one push listing a
    key twice, the int32 array with its negativity check, int64 first keys at 2^33 + 7
    and across 2^31, and alias keys."""
    run_case(oracle, case, lead)


@pytest.mark.parametrize("case", geom.separated_cases(), ids=lambda c: c["id"])
def test_separated_pushes(oracle, case):
    """One case per kernel family, each with at least two pushes, with 64 poison bytes
    between the pushes: an over-read that a neighbouring finite push would hide meets
    poison instead. (The split, the pre-reduce, its pieces and the big leaf have their
    own separated run: geom.PLACEMENTS.)"""
    run_case(oracle, case, 4, separated=True)


@pytest.mark.parametrize("place", geom.PLACEMENTS, ids=geom.placement_id)
def test_sparse_big_leaf_packed(oracle, place):
    """k_sp_leaf_big (the one-level sparse partition) on packed 12-byte records. The
    smallest shard with stats()["sparse_big_chunks"] == 1 for pushes that list each key
    once is 262 144 rows with 64 pushes of 180 000 keys (11.5 M records, a 138 MB arena;
    geom.BIG_LEAF has the arithmetic). A run takes 0.3 s on an MI355X (0.5 s for the
    first, which builds the pushes and the oracle's result once), so all four leads
    run, and once more with poison between the pushes."""
    from distml_amd import DataDesc, DataStore, KeyRange
    lead, separated = place
    c = geom.BIG_LEAF
    if "big_leaf" not in _REF:
        init, host, o = geom.big_leaf_case(oracle)
        _REF["big_leaf"] = (init, host, o.data.copy())
    init, host, want = _REF["big_leaf"]
    fmt = DataDesc(0, 1, 1)
    s = DataStore(fmt, KeyRange(c["first"], c["first"] + c["rows"] - 1), 1)
    try:
        s.load_values(init)
        a = geom.pack(host, lead, separated)
        s.stats(reset=True)
        s.pushDevice(a.ptrs, a.lens)
        s.flush()
        st = s.stats()
        assert s.error_state()[0] == 0
        assert st["sparse_big_chunks"] == 1 and st["sparse_replays"] == 0, st
        assert st["sparse_counted_chunks"] == 0, st  # no (big leaf, slice) region overflowed
        geom.kernel_is(s.kernel_name(), "k_sp_leaf_big")
        assert kat.bits_equal(s.values(), want)
        a.check()
    finally:
        s.close()


# --------------------------------------------------------------------------- split
@pytest.mark.parametrize("place", geom.PLACEMENTS, ids=geom.placement_id)
@pytest.mark.parametrize("case", geom.SPLIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_shard_split_packed(case, place):
    """dml_shard_split with packed inputs and the output at out_base + lead inside
    poison, out_cap exact: counts and bytes equal numpy's stable partition, and every
    byte before the output and after the kept bytes is still poison (k_split_scatter
    moves 16-byte chunks that straddle records). int64 keys: keys at total_rows + 2^32
    and at -2^32 + 5 are compared as 64-bit values and dropped. One run with poison
    between the pushes: a key read past a push's end would count a record less."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    lead, separated = place
    dtp, kt, vt, cols, total, world = case[:6]
    fmt = DataDesc(dtp, kt, vt)
    recs, K = geom.split_case(case)
    exp, exp_counts = geom.np_split(recs, K, total, world)
    a = geom.pack([r.tobytes() for r in recs], lead, separated)
    cap = sum(a.lens)
    out = geom.OutArena(cap, lead).upload()
    counts = HipOps().split(fmt, cols, total, world, a.ptrs, a.lens, out.ptr, cap,
                            torch.cuda.current_stream().cuda_stream)
    assert counts == exp_counts
    got = out.read()
    assert got[:len(exp)].tobytes() == exp
    out.untouched([(0, len(exp))])
    a.check()


# --------------------------------------------------------------------------- pre-reduce
@pytest.mark.parametrize("place", geom.PLACEMENTS, ids=geom.placement_id)
def test_prereduce_packed(oracle, place):
    """HipOps.prereduce (dml_reduce_buckets_dense) on packed full-range pushes, the
    output inside poison: bit-exact against an oracle store that starts at zero, and
    nothing outside the rows x cols output written. One run with poison between the
    pushes."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    lead, separated = place
    rows, cols, W = 1000, 300, 5
    fmt = DataDesc(1, 0, 1)
    host, want = _prereduce_ref(oracle, rows, cols, W)
    a = geom.pack(host, lead, separated)
    out = geom.OutArena(rows * cols * 4).upload()
    HipOps().prereduce(fmt, 0, rows, cols, a.ptrs, a.lens, out.ptr, torch.cuda.current_stream().cuda_stream)
    got = out.read()
    assert got.tobytes() == want.tobytes()
    out.untouched([(0, rows * cols * 4)])
    a.check()


def _prereduce_ref(oracle, rows, cols, W):
    key = ("prereduce", rows, cols, W)
    if key not in _REF:
        _REF[key] = geom.prereduce_case(oracle, rows, cols, W)
    return _REF[key]


@pytest.mark.parametrize("place", geom.PLACEMENTS, ids=geom.placement_id)
def test_prereduce_pieces_packed(oracle, place):
    """dml_prereduce_{begin,piece,end} with the 3-way split of
    test_prereduce_pieces_row_map on packed pushes. The two pieces write slabs 0 and 2
    of a poisoned three-slab output; slab 1, which no piece owns, and the guards stay
    poison. One run with poison between the pushes."""
    from distml_amd import DataDesc
    from distml_amd.group import HipOps
    lead, separated = place
    rows, cols, W, world, P = 1000, 300, 5, 3, 2
    S = (rows - 1 + world) // world
    blk = S // P
    fmt = DataDesc(1, 0, 1)
    host, want = _prereduce_ref(oracle, rows, cols, W)
    a = geom.pack(host, lead, separated)
    slab = world * blk * cols * 4
    out = geom.OutArena(3 * slab).upload()
    ops = HipOps()
    st = torch.cuda.current_stream().cuda_stream
    h = ops.begin(fmt, 0, rows, cols, a.ptrs, a.lens, st)
    for j in range(P):
        ops.piece(h, blk, S, j * blk, world * blk, out.ptr + 2 * j * slab, st)
    ops.end(h)
    got = out.read().view("<f4").reshape(3, world * blk, cols)
    for j in range(P):
        exp = np.zeros((world * blk, cols), np.float32)
        for t in range(world * blk):
            r = (t // blk) * S + j * blk + t % blk
            if r < rows:
                exp[t] = want[r]
        assert got[2 * j].tobytes() == exp.tobytes(), j
    out.untouched([(0, slab), (2 * slab, 3 * slab)])
    a.check()


# --------------------------------------------------------------------------- native group
def test_native_group_exchange_packed(oracle):
    """dml_group_push_exchange at world 1 with the caller's pushes packed (lead 4): two
    AdaGrad calls of key-subset pushes, some keys outside the matrix so the call splits
    and the store reads the slices back to back from the exchange buffer. Bit-exact
    data, alpha, delta and maxDelta."""
    from distml_amd import DataDesc
    from distml_amd.group import NativeShardGroup
    rows, cols = 1237, 200
    fmt = DataDesc(1, 0, 1, False, True, True)
    host, o = geom.exchange_case(oracle, rows, cols)
    g = NativeShardGroup(fmt, rows, cols, 0, 1, NativeShardGroup.unique_id(), device=0)
    try:
        g.store.setAlpha(*geom.ADA)
        a = geom.pack(host, 4)
        g.push_exchange(a.ptrs[:4], a.lens[:4])
        g.push_exchange(a.ptrs[4:], a.lens[4:])
        g.flush()
        assert kat.bits_equal(g.store.values(), o.data)
        al, de = g.store.adagrad_state()
        assert kat.bits_equal(al, o.alpha) and kat.bits_equal(de, o.delta)
        assert g.store.maxDelta() == o.max_delta()
        a.check()
    finally:
        g.close()


def test_native_group_full_range_packed(oracle):
    """dml_group_push_full_range at world 1 with the caller's pushes packed (lead 4):
    int32, two calls, exact (the reduce-scatter is a copy)."""
    from distml_amd import DataDesc
    from distml_amd.group import NativeShardGroup
    rows, cols, W = 1000, 256, 5
    fmt = DataDesc(1, 0, 0)
    host, o = geom.full_range_case(oracle, rows, cols, W)
    g = NativeShardGroup(fmt, rows, cols, 0, 1, NativeShardGroup.unique_id(), device=0, pieces=4)
    try:
        g.store.synth_fill(3)
        a = geom.pack(host, 4)
        g.push_full_range(a.ptrs[:3], a.lens[:3])
        g.push_full_range(a.ptrs[3:], a.lens[3:])
        g.flush()
        assert np.array_equal(g.store.values(), o.data)
        a.check()
    finally:
        g.close()


# --------------------------------------------------------------------------- alignment
def test_misaligned_pointers_refused_by_group_calls(oracle):
    """The native group's push calls check the pointers with their other arguments: a
    pointer that is 1 or 2 off gets DML_E_INVALID_ARG, the pre-reduce context and the
    store count no call, and the group then applies good calls exactly (int32, world 1)."""
    from distml_amd import DataDesc, NativeError, _lib
    from distml_amd.group import NativeShardGroup
    rows, cols, W = 1000, 256, 5
    fmt = DataDesc(1, 0, 0)
    host, o = geom.full_range_case(oracle, rows, cols, W)
    g = NativeShardGroup(fmt, rows, cols, 0, 1, NativeShardGroup.unique_id(), device=0, pieces=4)
    try:
        g.store.synth_fill(3)
        a = geom.pack(host, 4)
        before = g.store.stats()
        for skew in (1, 2):
            bad = [a.ptrs[0], a.ptrs[1] + skew]
            for call in (g.push_full_range, g.push_exchange, g.push_local):
                with pytest.raises(NativeError) as ei:
                    call(bad, a.lens[:2])
                assert ei.value.code == _lib.DML_E_INVALID_ARG
        g.flush()
        assert g.store.stats() == before and g.prereduce_stats()["chunks"] == 0
        g.push_full_range(a.ptrs[:3], a.lens[:3])
        g.push_full_range(a.ptrs[3:], a.lens[3:])
        g.flush()
        assert np.array_equal(g.store.values(), o.data)
        a.check()
    finally:
        g.close()


@pytest.mark.parametrize("skew", [1, 2])
def test_misaligned_device_pointers_are_refused(oracle, skew):
    """A device push pointer that is not 4-byte aligned gets DML_E_INVALID_ARG before
    any launch or state change, at every entry point that takes device pushes (the
    split also checks its output); the store's chunk count does not move and it still
    applies a good push exactly."""
    from distml_amd import DataDesc, DataStore, KeyRange, NativeError, _lib, encode_matrix_push
    from distml_amd.group import HipOps
    rows, cols = 301, 200
    fmt = DataDesc(1, 0, 1)
    rng = np.random.default_rng(5)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    push = encode_matrix_push(rng.permutation(rows), (rng.standard_normal((rows, cols)) * 1e-3).astype(np.float32), 0, 1)
    o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols)
    o.data[:] = init
    assert o.push(push) == 0
    a = geom.pack([push, push], 4)
    p, n = a.ptrs[0], a.lens[0]
    s = DataStore(fmt, KeyRange(0, rows - 1), cols)
    ops = HipOps()
    st = torch.cuda.current_stream().cuda_stream
    try:
        s.load_values(init)
        before = s.stats()
        for ptrs in ([p + skew], [p, a.ptrs[1] + skew]):
            with pytest.raises(NativeError) as ei:
                s.pushDevice(ptrs, [n] * len(ptrs))
            assert ei.value.code == _lib.DML_E_INVALID_ARG
        s.flush()
        assert s.stats() == before and s.error_state()[0] == 0
        assert kat.bits_equal(s.values(), init)
        out = geom.OutArena(rows * cols * 4).upload()
        with pytest.raises(NativeError) as ei:
            ops.prereduce(fmt, 0, rows, cols, [p + skew], [n], out.ptr, st)
        assert ei.value.code == _lib.DML_E_INVALID_ARG
        with pytest.raises(NativeError) as ei:
            ops.begin(fmt, 0, rows, cols, [p + skew], [n], st)
        assert ei.value.code == _lib.DML_E_INVALID_ARG
        ctx = ops.ctx_create(fmt, 0, rows, cols, 0)
        try:
            with pytest.raises(NativeError) as ei:
                ops.begin_ctx(ctx, [p + skew], [n], st)
            assert ei.value.code == _lib.DML_E_INVALID_ARG
            assert ops.ctx_stats(ctx)["chunks"] == 0
        finally:
            ops.ctx_destroy(ctx)
        for ptrs, optr in (([p + skew], out.ptr), ([p], out.ptr + skew)):
            with pytest.raises(NativeError) as ei:
                ops.split(fmt, cols, rows, 2, ptrs, [n], optr, n, st)
            assert ei.value.code == _lib.DML_E_INVALID_ARG
        out.read()
        out.untouched([])
        s.pushDevice([p], [n])
        s.flush()
        assert s.stats()["chunks"] == before["chunks"] + 1
        assert kat.bits_equal(s.values(), o.data)
        a.check()
    finally:
        s.close()

"""Pins tests/geom.py without a GPU: the packed layout, the poison word under every
reading, and that the oracle alone, on the unpacked pushes of every case of
tests/test_gpu_geometry.py, gives finite values and no error. With that pinned, a NaN
or an unexpected error on the GPU can only come from a read outside a push."""
import numpy as np
import pytest

import geom


@pytest.mark.parametrize("separated", [False, True])
@pytest.mark.parametrize("lead", geom.LEADS)
def test_layout_offsets(lead, separated):
    pushes = [bytes([b + 1]) * n for b, n in enumerate((804 * 3, 4004, 12 * 7, 16, 8))]
    a = geom.Arena(pushes, lead, separated)
    assert a.offs[0] == geom.GUARD + lead and a.offs[0] % 16 == lead
    run = lead
    for i, (o, n) in enumerate(zip(a.offs, a.lens)):
        if i and separated:
            run += geom.GAP
        assert o == geom.GUARD + run and o % 16 == run % 16 and o % 4 == 0
        assert a.host[o:o + n].tobytes() == pushes[i]
        run += n
    if not separated:  # back to back: no byte between two pushes
        assert all(a.offs[i] + a.lens[i] == a.offs[i + 1] for i in range(len(pushes) - 1))
    else:
        for i in range(len(pushes) - 1):
            gap = a.host[a.offs[i] + a.lens[i]:a.offs[i + 1]]
            assert gap.size == geom.GAP and (gap.view("<u4") == geom.POISON).all()
    end = a.offs[-1] + a.lens[-1]
    assert a.host.size - end >= geom.GUARD and a.host.size % 16 == 0
    # the guard mask is exactly the complement of the pushes, and all of it is poison
    assert int((~a.guard).sum()) == sum(a.lens)
    g = a.host.copy()
    for o, n in zip(a.offs, a.lens):
        g[o:o + n] = np.frombuffer(np.array([geom.POISON], "<u4").tobytes() * (n // 4), np.uint8)
    assert (g.view("<u4") == geom.POISON).all()
    assert a.guard[:geom.GUARD + lead].all() and a.guard[end:].all()


@pytest.mark.parametrize("lead", geom.LEADS)
def test_out_arena_layout(lead):
    o = geom.OutArena(4004 * 3, lead)
    assert o.off == geom.GUARD + lead and o.host.size - o.off - o.nbytes >= geom.GUARD
    assert (o.host.view("<u4") == geom.POISON).all()


def test_poison_readings():
    assert np.isnan(geom.poison_f32()) and np.isnan(geom.poison_f64())
    assert geom.poison_i32() == 0x7FF7FFFF == 2_146_959_359
    assert geom.poison_i64() == 0x7FF7FFFF7FF7FFFF
    # no test sum absorbs it: counters start below 200 and move by at most 2 per push
    assert geom.poison_i32() > 1 << 30


def test_row_index_is_the_oracles(oracle):
    """geom.row_index against the oracle's own narrowing, through a 1-column store."""
    from distml_amd.store import encode_matrix_push
    for first in (0, 1000, geom.NEG32, geom.BIG33, geom.STRADDLE):
        for key in (first, first + 99, first + 100, first - 1, first + 5 + geom.ALIAS, first + 5 - geom.ALIAS,
                    geom.POISON, geom.poison_i64()):
            o = oracle.OracleStore(1, 1, 3, first, first + 99, 1)
            rc = o.push(encode_matrix_push([key], [[1.0]], 1, 3))
            r = geom.row_index(key, first, 100)
            assert (rc == 0) == (r >= 0), (first, key)
            if r >= 0:
                assert o.data[r, 0] == 1.0 and o.data.sum() == 1.0


@pytest.mark.parametrize("case", geom.ALL_CASES, ids=lambda c: c["id"])
def test_case_oracle_alone_is_finite(oracle, case):
    """The case's pushes, unpacked: no error, finite values; the poison key is outside
    the case's shard; the alias keys really are 2^32 away from an in-shard key."""
    assert geom.poison_row(case["first"], case["rows"]) == -1
    init, pushes, o, rc = geom.oracle_run(case, oracle)
    assert rc == 0 and o.error()[0] == 0
    assert not np.array_equal(o.data, init)
    if case["vt"] != 0:
        assert np.isfinite(o.data).all()
    else:
        assert (o.data >= 0).all() and (o.data < 1000).all()
    if case["ada"]:
        assert np.isfinite(o.alpha).all() and np.isfinite(o.delta).all() and (o.delta > 1.0).any()
    K = 4 if case["kt"] == 0 else 8
    stride = K + (8 if case["vt"] == 3 else 4) * case["cols"]
    last = case["first"] + case["rows"] - 1
    nalias = 0
    for p in pushes:
        assert len(p) % stride == 0 and len(p) % 4 == 0
        k = np.frombuffer(p, np.uint8).reshape(-1, stride)[:, :K].copy().view("<i4" if K == 4 else "<i8").ravel()
        out = (k < case["first"]) | (k > last)
        nalias += int(out.sum())
        assert all(geom.row_index(int(x), case["first"], case["rows"]) >= 0 for x in k[out])
    assert nalias == (3 if case["alias"] else 0)


def test_other_cases_oracle_alone_is_finite(oracle):
    """The pre-reduce, exchange, full-range and big-leaf inputs, unpacked: no error (the
    builders assert it) and finite / non-negative results; poison keys outside them."""
    host, want = geom.prereduce_case(oracle)
    assert np.isfinite(want).all() and len(host) == 5 and geom.poison_row(0, 1000) == -1
    host, o = geom.exchange_case(oracle)
    assert np.isfinite(o.data).all() and np.isfinite(o.alpha).all() and np.isfinite(o.delta).all()
    assert o.error()[0] == 0 and geom.poison_row(0, 1237) == -1
    host, o = geom.full_range_case(oracle)
    assert o.error()[0] == 0 and (o.data >= 0).all()
    init, host, o = geom.big_leaf_case(oracle)
    assert o.error()[0] == 0 and np.isfinite(o.data).all() and not np.array_equal(o.data, init)
    assert geom.poison_row(geom.BIG_LEAF["first"], geom.BIG_LEAF["rows"]) == -1
    # the planner's conditions for the one-level partition (sparse_plan_big)
    nrec = geom.BIG_LEAF["n"] * geom.BIG_LEAF["per"]
    nbig = geom.BIG_LEAF["rows"] >> 4
    assert nbig == 16384 and 4096 // 6 <= nrec // nbig <= 4096 * 17 // 24 and geom.BIG_LEAF["n"] >= 8


def test_separated_families_cover_every_kernel():
    """Every family has a separated case, and each has a gap: at least two pushes, so
    its separated arena differs from the packed one."""
    for c in geom.separated_cases():
        assert c["n"] >= 2, c["id"]
        lens = [804] * c["n"]
        assert geom.layout(lens, 4, True)[0] != geom.layout(lens, 4, False)[0]
    assert {f for f in (c["family"] for c in geom.ALL_CASES)} == {c["family"] for c in geom.separated_cases()}
    assert (4, True) in geom.PLACEMENTS and [p[0] for p in geom.PLACEMENTS if not p[1]] == list(geom.LEADS)
    fam = {c["family"] for c in geom.separated_cases()}
    assert {"k_reduce", "k_reduce_rows", "k_reduce_flat", "k_flat_ident", "k_ada_flat", "k_ada_ident",
            "k_reduce_ada", "k_sp_leaf", "alias"} <= fam


@pytest.mark.parametrize("case", geom.SPLIT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_case_poison_is_dropped(case):
    """dml_shard_split compares whole 64-bit keys against [0, total_rows): a key made
    of poison (int32, or either or both words of an int64) is outside every tuple's
    matrix, so a key read outside a push changes the counts; the alias keys the int64
    tuples plant are dropped by numpy's reference too."""
    total, K = case[4], (4 if case[1] == 0 else 8)
    for key in (geom.poison_i32(), geom.POISON, geom.poison_i64(), geom.POISON << 32, (geom.POISON << 32) | 5):
        assert not geom.split_owner(key, total)
    recs, K2 = geom.split_case(case)
    assert K2 == K and len(recs) == case[6]
    exp, counts = geom.np_split(recs, K, total, case[5])
    kept = sum(map(sum, counts))
    assert 0 < kept < sum(len(r) for r in recs) and len(exp) == kept * recs[0].shape[1]
    if K == 8:
        for r in recs:
            k = r[:, :8].copy().view("<i8").ravel()
            assert (k == total + (1 << 32)).any() and (k == 5 + (1 << 32)).any() and (k == 5 - (1 << 32)).any()


def test_kernel_name_fields():
    n = "dml::k_reduce_rows<float, 0, 4, 4, true, true, 1, 4, 2>"
    geom.kernel_is(n, "k_reduce_rows", type="float", CPW=4, FULL="true", DEPTH=1)
    with pytest.raises(AssertionError):
        geom.kernel_is(n, "k_reduce_rows", DEPTH=3)
    with pytest.raises(AssertionError):
        geom.kernel_is(n, "k_reduce")
    geom.kernel_is("dml::k_flat_ident<double, 0, 8, 3, 8>", "k_flat_ident", type="double")
    geom.kernel_is("dml::k_sp_leaf_big", "k_sp_leaf_big")

"""CPU checks of the sparse route model (tests/sparse_route.py) and of the GPU case table
(tests/sparse_cases.py); no GPU needed.

1. The model's plan equals the library's own (dml_diag_sparse_plan, which calls the functions
   launch_chunk and launch_sparse_leaf call) field for field over a sweep of shard sizes, push
   counts, record totals, shares, value types and the tail cut.
2. Every case of the table is on the route it declares, and the two members of every boundary
   pair differ in exactly the predicate the pair is about. No exceptions: this is what keeps
   tests/test_gpu_sparse_edges.py from quietly testing another route.
3. The cases whose point is the order of adds give other bits when the oracle applies their
   records in another order.
Running with -s prints the route-by-type matrix of the table (pasted into DESIGN.md §4.5).
"""
import ctypes as C

import numpy as np
import pytest

import sparse_cases as SC
import sparse_route as R


def lib_plan(vt, rows, nrecs, tail_cut):
    from distml_amd import _lib
    L = _lib.load()
    a = (C.c_int64 * len(nrecs))(*nrecs)
    o = _lib.dml_sparse_plan_info()
    assert L.dml_diag_sparse_plan(vt, rows, a, len(nrecs), int(tail_cut), C.byref(o)) == 0, _lib.last_error()
    return {f: getattr(o, f) for f in R.FIELDS}


def shares(total, nb, kind):
    if kind == "equal":
        w = [1] * nb
    elif kind == "double":  # one push twice the others: the smax * 8 > nrec * 5 / 4 refusal at 8 pushes
        w = [2] + [1] * (nb - 1)
    else:                   # ramp
        w = list(range(1, nb + 1))
    out = [total * x // sum(w) for x in w]
    out[-1] += total - sum(out)
    return out


def sweep():
    rows_set = set()
    for k in range(31):
        rows_set |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    rows_set |= {3 * 5 * 7 * 11, 131_088, 262_144 + 12_345, 1_048_704, 99_999_999, (1 << 31) - 1}
    for rows in sorted(r for r in rows_set if 1 <= r <= (1 << 31) - 1):
        totals = set()
        for k in range(0, 38):
            totals |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
        totals = sorted(t for t in totals if 1 <= t <= 64 * rows)
        for i, total in enumerate(totals):
            for j, nb in enumerate((1, 7, 8, 9, 63, 64)):
                yield rows, shares(total, nb, ("equal", "double", "ramp")[(i + j) % 3])
        # the big-leaf window (mean 682 .. 2 901 records per big leaf), where the shares decide
        BL = 0
        while BL < 24 and ((rows + (1 << BL) - 1) >> BL) > R.K_BIG_BINS:
            BL += 1
        nbig = (rows + (1 << BL) - 1) >> BL
        for mean in (681, 682, 1500, 2901, 2902):
            for nb in (7, 8, 9, 64):
                for kind in ("equal", "double", "ramp"):
                    yield rows, shares(mean * nbig + nbig // 2, nb, kind)


def test_plan_model_equals_library():
    n = nbig = 0
    for rows, nrecs in sweep():
        for vt in (R.F32, R.F64, R.I32):
            for tail in (False, True):
                want = R.plan(vt, rows, nrecs, tail)
                got = lib_plan(vt, rows, nrecs, tail)
                assert got == want, (vt, rows, nrecs, tail, got, want)
                n += 1
                nbig += want["big"]
    print(f"\n{n} plans compared, {nbig} of them big-leaf plans")
    assert n > 20_000 and nbig > 100


def test_big_plan_never_refused_for_BL_below_SL():
    """sparse_plan_big's `BL < SL` refusal (dml_sparse.hip:1058) cannot be reached: a mean of at
    least kSpBigCap / 6 = 682 records per big leaf of 2^BL rows bounds sparse_plan's span,
    1024 * rows / nrec, by 1024 * 2^BL / 682 < 2^(BL + 1), so SL <= BL, and the 65 536-leaf
    loop stops at or below BL because rows >> BL <= 16 384. So the table has no such GPU case;
    this pins the arithmetic instead, over every plan of the sweep that passes the mean test."""
    seen = 0
    for rows, nrecs in sweep():
        p = R.plan(R.F32, rows, nrecs)
        if not p["compact"] or len(nrecs) < R.K_SLICES:
            continue
        BL = 0
        while BL < 24 and ((rows + (1 << BL) - 1) >> BL) > R.K_BIG_BINS:
            BL += 1
        mean = p["nrec"] // ((rows + (1 << BL) - 1) >> BL)
        if R.K_BIG_CAP // 6 <= mean <= R.K_BIG_CAP * 17 // 24:
            seen += 1
            assert BL >= p["SL"], (rows, nrecs, BL, p)
    assert seen > 100


def test_bad_arguments_are_refused():
    from distml_amd import _lib
    L = _lib.load()
    o = _lib.dml_sparse_plan_info()
    one = (C.c_int64 * 65)(*([1] * 65))
    for vt, rows, n in ((2, 10, 1), (1, 0, 1), (1, 10, 0), (1, 10, 65), (1, 1 << 31, 1)):
        assert L.dml_diag_sparse_plan(vt, rows, one, n, 0, C.byref(o)) == _lib.DML_E_INVALID_ARG
    assert L.dml_diag_sparse_plan(1, 10, None, 1, 0, C.byref(o)) == _lib.DML_E_INVALID_ARG


def _declared(r):
    kinds = sorted({k for v in r["flagged"].values() for k, _ in v})
    return dict(big=r["big"], compact=r["compact_at_launch"], counted=tuple(sorted(r["why"])), flagged=tuple(kinds),
                branch=r["replay_branch"])


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["id"])
def test_case_is_on_its_route(case):
    rs = SC.routes(case)
    assert len(rs) == len(case["claims"])
    for r, claim in zip(rs, case["claims"]):
        want = dict(claim, counted=tuple(sorted(claim["counted"])), flagged=tuple(sorted(claim["flagged"])))
        assert _declared(r) == want, (case["id"], r["plan"], r["why"], r["flagged"])
    if case["check"]:
        assert case["check"](rs[0]["plan"]), rs[0]["plan"]
    # the planned error is what the keys hold: a cutoff exactly when a key lies outside the shard
    b = SC.built(case)
    outside = any((R.row_index(k, case["first"], case["rows"]) < 0).any() for k in b["keys"])
    assert (rs[0]["seq_cut"] is not None) == (outside or b["trunc"] is not None)
    assert (case["err"] in ("key", "trunc")) == (rs[0]["seq_cut"] is not None) or case["err"] == "neg"
    if case["order"]:
        assert all(0 <= r < case["rows"] for r in case["order"])
    # the chunk that follows on the same store is an ordinary one: single pass, nothing flagged
    r2 = R.route(case["vt"], case["first"], case["rows"], b["keys2"])
    assert not r2["counted"] and not r2["flagged"] and not r2["big"], (r2["why"], r2["flagged"])


@pytest.mark.parametrize("case", [c for c in SC.CASES if c["pair"]], ids=lambda c: c["id"])
def test_boundary_pair_differs_in_one_predicate(case):
    other = SC.BY_ID[case["pair"]]
    a, b = SC.routes(case)[0], SC.routes(other)[0]
    pa, pb = R.predicates(a), R.predicates(b)
    diff = sorted(k for k in pa if pa[k] != pb[k])
    assert diff == sorted(case["flips"]), (case["id"], other["id"], pa, pb)
    # same shape, same plan where the pair is not about the plan itself
    if "compact_at_launch" not in case["flips"] and "big" not in case["flips"]:
        assert a["plan"] == b["plan"]
    # the capacity is hit exactly: the fuller member is one record over, the other one exactly full
    for cap in ("cap1", "cap2", "capS"):
        if cap in case["flips"]:
            assert list(b["why"][cap].values()) == [a["plan"][cap] + 1]
            assert _max_count(case, a, cap) == a["plan"][cap]
    if case["flips"] == ("bucket",):
        assert {n for v in b["flagged"].values() for k, n in v if k == "bucket"} == {R.K_BUCKET_MAX + 1}
        assert _max_bucket(case, a) == R.K_BUCKET_MAX
    if "leaf_records" in case["flips"]:
        cap = R.K_BIG_CAP if b["big"] and not b["counted"] else R.K_LEAF_CAP
        assert {n for v in b["flagged"].values() for k, n in v if k == "records"} == {cap + 1}
        if b["big"]:
            assert _max_count(case, a, "big_leaf") == cap


def _rows_of(case):
    b = SC.built(case)
    row = np.concatenate([R.row_index(k, case["first"], case["rows"]) for k in b["keys"][:R.K_MAX_W]])
    push = np.repeat(np.arange(len(b["keys"][:R.K_MAX_W])), [len(k) for k in b["keys"][:R.K_MAX_W]])
    return row[row >= 0], push[row >= 0]


def _max_count(case, r, cap):
    p = r["plan"]
    row, push = _rows_of(case)
    ids = {"cap1": (row >> p["SL"]) >> p["D2"], "cap2": row >> p["SL"], "big_leaf": row >> p["BL"],
           "capS": (row >> p["BL"]) * R.K_SLICES + push % R.K_SLICES}[cap]
    return int(np.unique(ids, return_counts=True)[1].max())


def _max_bucket(case, r):
    p = r["plan"]
    row, _ = _rows_of(case)
    sh = p["BL"] if p["big"] else p["SL"]
    ids = ((row >> sh) << 32) | ((row - ((row >> sh) << sh)) >> p["bshift"])
    return int(np.unique(ids, return_counts=True)[1].max())


def _applied(case):
    """The case's records the reference applies, per push: everything before the first key outside
    the shard (a ragged tail holds no record)."""
    b = SC.built(case)
    keys, vals = [], []
    for k, v in zip(b["keys"], b["vals"]):
        bad = np.flatnonzero(R.row_index(k, case["first"], case["rows"]) < 0)
        n = int(bad[0]) if len(bad) else len(k)
        keys.append(k[:n])
        vals.append(v[:n])
        if len(bad):
            break
    return keys, vals


def _oracle_rows(oracle, case, order):
    """The oracle's values of the case's `order` rows with its applied records added in `order`."""
    b = SC.built(case)
    o = SC.oracle_store(oracle, case)
    o.data[:] = b["init"]
    keys, vals = _applied(case)
    if order == "reversed":  # last push first, every push's records last first
        keys, vals = [k[::-1] for k in keys[::-1]], [v[::-1] for v in vals[::-1]]
    elif order == "by_row":  # one push, sorted by row, then by value
        k, v = np.concatenate(keys), np.concatenate(vals)
        i = np.lexsort((v, k))
        keys, vals = [k[i]], [v[i]]
    elif order == "by_row_desc":  # the same, values descending
        k, v = np.concatenate(keys), np.concatenate(vals)
        i = np.lexsort((-v, k))
        keys, vals = [k[i]], [v[i]]
    elif order == "swap":  # only the two same-push records of one row change places
        p, i, j = b["swap"]
        vals = [v.copy() for v in vals]
        vals[p][[i, j]] = vals[p][[j, i]]
    for p in SC.encode(case, keys, vals):
        assert o.push(p) == 0
    out = o.data[list(case["order"]), 0].copy()
    o.close()
    return out


@pytest.mark.parametrize("case", [c for c in SC.CASES if c["order"] and c["vt"] != R.I32], ids=lambda c: c["id"])
def test_yardstick_tells_orders_apart(oracle, case):
    """Every `order` row of the case gets other bits from the oracle when the applied records are
    added in reversed order or sorted by (row, value): a kernel that added any of these rows in
    another order would fail the byte comparison of the GPU test. The rows lie where the case's
    point is: in the flagged leaf or bucket of the replayed cases (checked against the model).
    Where one push lists a row twice, changing the places of just those two records changes that
    row's bits too: this is the order only full sequence numbers keep. (int32 adds commute.)"""
    want = _oracle_rows(oracle, case, "push")
    alts = [_oracle_rows(oracle, case, o) for o in ("reversed", "by_row", "by_row_desc")]
    assert np.isfinite(want).all()
    for n, row in enumerate(case["order"]):
        assert any(want[n].tobytes() != a[n].tobytes() for a in alts), (case["id"], row)
    r = SC.routes(case)[0]
    if r["flagged"]:
        lsh = r["plan"]["BL"] if r["big"] and not r["counted"] else r["plan"]["SL"]
        assert {row >> lsh for row in case["order"]} <= set(r["flagged"]), (case["id"], r["flagged"])
    swap = SC.built(case)["swap"]
    if swap:
        p, i, j = swap
        row = int(SC.built(case)["keys"][p][i] - case["first"])
        assert row in case["order"] and SC.built(case)["keys"][p][j] - case["first"] == row
        sw = _oracle_rows(oracle, case, "swap")
        n = case["order"].index(row)
        assert want[n].tobytes() != sw[n].tobytes(), (case["id"], row)


def test_same_push_repeats_have_a_swap_yardstick():
    """Every float case in which one push lists a row twice names the two records as its `swap`."""
    for c in SC.CASES:
        b = SC.built(c)
        twice = any(len(np.unique(k)) < len(k) for k in b["keys"][:R.K_MAX_W]) if not c["heavy"] else False
        assert bool(b["swap"]) == twice, c["id"]


def test_route_matrix_reaches_every_branch():
    """Across the table every replay branch is reached for each value type that can take it
    (1 and 2: fp32 only, compact words; 3 and 4: all three), every capacity is hit exactly full
    and one over, and both layouts run for every type. Prints the matrix (pytest -s)."""
    cell = {}
    for c in SC.CASES:
        for r in SC.routes(c):
            t = SC.TAG[c["vt"]]
            part = "big" if r["big"] and not r["counted"] else "counted" if r["counted"] else \
                "single-pass compact" if r["compact_at_launch"] else "single-pass full"
            cell.setdefault((f"partition: {part}", t), []).append(c["id"])
            for w in r["why"]:
                cell.setdefault((f"counted because: {w}", t), []).append(c["id"])
            if r["replay_branch"]:
                cell.setdefault((f"replay branch {r['replay_branch']}", t), []).append(c["id"])
            if r["seq_cut"] is not None and r["replay_branch"]:
                cell.setdefault(("replay under a cutoff", t), []).append(c["id"])
    lines = ["| route | f32 | f64 | i32 |", "|---|---|---|---|"]
    for name in sorted({k[0] for k in cell}):
        cols = []
        for t in ("f32", "f64", "i32"):
            ids = sorted({i.rsplit("-", 1)[0] for i in cell.get((name, t), [])})
            cols.append(", ".join(ids) if ids else "-")
        lines.append(f"| {name} | " + " | ".join(cols) + " |")
    print("\n" + "\n".join(lines))
    for t in ("f32", "f64", "i32"):
        assert cell.get(("replay branch 3", t)) or t == "f32"
        assert cell.get(("replay branch 4", t))
        assert cell.get(("partition: counted", t))
    for b in SC.REQUIRED_F32_BRANCHES:
        assert cell.get((f"replay branch {b}", "f32")), b
    assert not cell.get(("replay branch 1", "f64")) and not cell.get(("replay branch 2", "i32"))

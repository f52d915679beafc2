"""The sparse array path (dml_sparse.hip) on the capacity comparisons and replay branches that
random keys never reach, against the CPU oracle byte for byte.

The cases are tests/sparse_cases.py's table: every one is built at the smallest shape that puts
a record count exactly on, or one past, cap1 / cap2 / capS, the leaf capacities and the line
bucket limit, or that sends a flagged leaf through one of sparse_replay's four branches, with
and without a cutoff and an int32 negative counter. tests/test_sparse_route.py proves without a
GPU that each case is on the route it declares (tests/sparse_route.py restates the plan and
the kernels' counting); here the store must
  - equal the oracle (pyoracle.OracleStore) byte for byte, tobytes() against tobytes(),
  - report the oracle's error state (code, key, col) where the case plans an error,
  - count sparse_big_chunks, sparse_counted_chunks and sparse_replays as the model predicts and
    name the leaf kernel it predicts (dml_store_kernel_name),
  - and apply a following small chunk exactly too: it reuses the workspace under another layout.
A case whose chunk is counted or replayed runs through both handlePushBatch and pushDevice, the
others through one of the two (the id's checksum picks it); pushDevice takes a packed arena
(tests/geom.py: pushes back to back at 4-byte-aligned addresses between poisoned guards).

Values include +-0.0, denormals, the largest finite numbers and +-Inf; +Inf and -Inf are kept on
different rows, so no NaN arises: x86's and the GPU's default NaN differ in sign, which is not
what these cases are about.
"""
import numpy as np
import pytest

import geom
import sparse_cases as SC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR = {"key": 2, "trunc": 3, "neg": 4}  # DML_E_KEY_OUT_OF_SHARD, DML_E_TRUNCATED, DML_E_NEGATIVE_COUNTER


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


_REF = {}


def reference(oracle, case):
    """The case's encoded pushes and the oracle's state after them and after the following chunk;
    once per case."""
    if case["id"] not in _REF:
        if case["heavy"]:  # tens of MB each: only the latest stays
            for k in [k for k in _REF if SC.BY_ID[k]["heavy"]]:
                del _REF[k]
        b = SC.built(case)
        pushes = SC.encode(case, b["keys"], b["vals"], b["trunc"])
        more = SC.encode(case, b["keys2"], b["vals2"])
        o = SC.oracle_store(oracle, case)
        o.data[:] = b["init"]
        err = (0, 0, -1)
        for p in pushes:
            if o.push(p):
                err = o.error()
                break
        after = o.data.copy()
        o.clear_error()
        for p in more:
            assert o.push(p) == 0
        _REF[case["id"]] = dict(pushes=pushes, more=more, err=err, after=after, final=o.data.copy())
        o.close()
    return _REF[case["id"]]


def _push(s, fmt, pushes, api):
    """One call with all the pushes; returns the arena to check (device entry) or None."""
    if api == "batch":
        s.handlePushBatch(fmt, pushes)
        return None
    a = geom.pack(pushes, 4)
    s.pushDevice(a.ptrs, a.lens)
    s.flush()
    return a


@pytest.mark.parametrize("case,api", [(c, a) for c in SC.CASES for a in SC.apis(c)],
                         ids=lambda x: x["id"] if isinstance(x, dict) else x)
def test_sparse_edge(oracle, case, api):
    from distml_amd import DataDesc, DataStore, DistMLException, KeyRange
    ref = reference(oracle, case)
    routes = SC.routes(case)
    want = {k: sum(r["counters"][k] for r in routes) for k in routes[0]["counters"]}
    assert (ref["err"][0] != 0) == (case["err"] is not None), ref["err"]
    if case["err"]:
        assert ref["err"][0] == ERR[case["err"]], ref["err"]
    fmt = DataDesc(0, case["kt"], case["vt"])
    s = DataStore(fmt, KeyRange(case["first"], case["first"] + case["rows"] - 1), 1)
    try:
        s.load_values(SC.built(case)["init"])
        s.stats(reset=True)
        if case["err"]:
            with pytest.raises(DistMLException) as ei:
                a = _push(s, fmt, ref["pushes"], api)
            a = None
            assert (ei.value.code, ei.value.key, ei.value.col) == ref["err"]
            assert s.error_state() == ref["err"]
        else:
            a = _push(s, fmt, ref["pushes"], api)
            assert s.error_state()[0] == 0
        st = s.stats(reset=True)
        name = s.kernel_name()
        got = s.values()
        print(case["id"], api, name, {k: st[k] for k in want}, routes[0]["why"], routes[0]["flagged"])
        assert got.tobytes() == ref["after"].tobytes(), (case["id"], name, st, _first_diff(got, ref["after"]))
        assert {k: st[k] for k in want} == want, (st, want)
        assert name == routes[-1]["kernel"], (name, routes[-1]["kernel"])
        if a is not None:
            a.check()
        # a following small, ordinary chunk: the workspace under another layout
        s.clear_error()
        a2 = _push(s, fmt, ref["more"], api)
        got = s.values()
        assert got.tobytes() == ref["final"].tobytes(), (case["id"], "following chunk", _first_diff(got, ref["final"]))
        st2 = s.stats()
        assert (st2["sparse_counted_chunks"], st2["sparse_replays"], st2["sparse_big_chunks"]) == (0, 0, 0), st2
        if a2 is not None:
            a2.check()
    finally:
        s.close()


def _first_diff(got, want):
    g, w = got.ravel(), want.ravel()
    bad = np.flatnonzero(g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1))
    rows = np.unique(bad // g.itemsize)
    if not len(rows):
        return None
    r = int(rows[0])
    return dict(rows_differing=int(len(rows)), row=r, got=g[r].item(), want=w[r].item())

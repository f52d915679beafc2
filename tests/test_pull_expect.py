"""CPU: tests/pull_expect.py, the yardstick of the collective group pull, on the exact inputs
the GPU tests use (tests/test_native_pull.py). Passes without the feature, by design: it
shows that the expected bytes tell the cases apart."""
import numpy as np
import pytest

import pull_expect as P


@pytest.mark.parametrize("tag,world", P.TABLE, ids=[f"{t}-w{w}" for t, w in P.TABLE])
def test_table_expectations(oracle, tag, world):
    """Per rank: counts sum to the kept keys, the lengths follow, dropped keys leave no record,
    a repeated key has one record per occurrence, and (where a rank asks more than one owner
    out of list order) the two output orders differ."""
    rec = P.record_bytes(tag)
    lists = P.key_lists(tag, world)
    rows = P.SPECS[tag][4]
    differ = False
    for r, (om, rq, counts) in enumerate(P.table_expected(oracle, tag, world)):
        keys = lists[r]
        kept = [int(k) for k in keys if 0 <= k < rows]
        assert sum(counts) == len(kept) and len(om) == len(rq) == len(kept) * rec
        K = 4 + 4 * P.SPECS[tag][1]
        rq_keys = np.frombuffer(rq, np.uint8).reshape(-1, rec)[:, :K].copy().view("<i4" if K == 4 else "<i8").ravel()
        assert rq_keys.tolist() == kept  # request order: record j is the j-th kept key's
        om_keys = np.frombuffer(om, np.uint8).reshape(-1, rec)[:, :K].copy().view("<i4" if K == 4 else "<i8").ravel()
        assert om_keys.tolist() == [k for q in P.split(tag, world, keys) for k in q]
        assert sorted(np.frombuffer(om, np.uint8).reshape(-1, rec).tolist()) == \
            sorted(np.frombuffer(rq, np.uint8).reshape(-1, rec).tolist())
        differ = differ or om != rq
    assert differ == (world > 1)  # every world > 1 has a rank whose list is not owner-ordered


def test_split_is_keyrange_intersect():
    """For a list without repeats the split is KeyRange.intersect(KeyList), list order kept."""
    from distml_amd.datadesc import KeyList
    keys = np.array([999, -1, 668, 1000, 5, 334, 1 << 40, 0, 667, 333, -(1 << 33), (1 << 32) + 5], np.int64)
    per = P.split("f32c67", 3, keys)
    for p, got in zip(P.parts("f32c67", 3), per):
        assert got == list(p.intersect(KeyList(keys.tolist())))
    assert per == [[5, 0, 333], [334, 667], [999, 668]]


def test_key_list_kinds():
    kinds = {k for w in P.KINDS.values() for k in w}
    assert kinds == {"edges", "desc700", "own257", "remote257", "remote1", "empty"}
    assert [len(P.key_list(k, "f32c67", 4, 1)) for k in ("desc700", "own257", "remote1", "empty")] == [700, 257, 1, 0]
    e = P.key_list("edges", "f32c67", 3, 0)
    assert {-1, 1000, 1 << 40, 0, 333, 334, 667, 668, 999} <= set(e.tolist())
    assert (e == 0).sum() == 2 and (e == 999).sum() == 2  # repeats
    d = P.key_list("desc700", "f32c67", 2, 0)
    assert (np.diff(d[:643]) == -1).all() and d[643:].tolist() == d[:57].tolist()
    own = P.key_list("own257", "f32c67", 3, 1)
    assert ((own >= 334) & (own <= 667)).all() and len(set(own.tolist())) < 257
    rem = P.key_list("remote257", "f32c768k8", 4, 2)
    assert ((rem >= 150) & (rem <= 199)).all()


@pytest.mark.parametrize("case", sorted(P.ORDER))
def test_ordering_expectations(oracle, case):
    """The first pull holds the first push's state only: on every rank that asks for anything,
    the bytes before and after the second push differ."""
    first, second = P.order_expected(oracle, case)
    tag, world, _ = P.ORDER[case]
    asked = 0
    for r in range(world):
        assert first[r][2] == second[r][2]
        if sum(first[r][2]):
            asked += 1
            assert first[r][0] != second[r][0] and first[r][1] != second[r][1]
    assert asked >= 1


def test_closed_shard_expectation(oracle):
    """Shard 1 closed in call 0: its rows hold the adds up to the failing one, so they differ
    from the start values and from a run in which the shard had taken everything."""
    from chain_i32_expect import group_calls, init_counts
    tag, world = P.CLOSED
    rows, cols = P.SPECS[tag][4], P.SPECS[tag][5]
    got = P.closed_expected(oracle)
    m = P.Model(oracle, tag, world, init_counts(rows, cols))
    start = m.pulls(P.key_lists(tag, world))
    m.close()
    assert got[1][0] != start[1][0]  # rank 1 asks its own, closed shard
    clean = P.Model(oracle, tag, world, init_counts(rows, cols))
    clean.chained(group_calls(world, rows, cols, "chain")[0])
    assert clean.closed == [False] * 3
    clean.close()

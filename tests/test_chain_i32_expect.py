"""CPU: the int32 chain's yardstick (tests/chain_i32_expect.py) tells things apart on
exactly the inputs the GPU tests use."""
import numpy as np
import pytest

import chain_expect as X
import chain_i32_expect as E

COLS = 67  # any width: the yardstick's verdicts do not depend on the kernel shape


@pytest.mark.parametrize("W,kind", [(1, "perm"), (11, "asc"), (11, "subset"), (64, "perm")])
def test_clean_cases_report_no_error(oracle, W, kind):
    """64 + h % 51 with deltas down to -2 would not survive 33 adds; init_counts starts at 1000."""
    cols = 3 if W == 64 else COLS
    calls = E.calls_of(E.WORLD, W, E.ROWS, cols, 2 if W < 64 else 1, kind, short=lambda r, c: (r, c) == (0, 1))
    init = E.init_counts(E.ROWS, cols)
    want = E.expected(oracle, E.WORLD, E.ROWS, cols, calls, init)
    assert [e for _, e in want] == [(0, 0, -1)] * E.WORLD
    assert min(int(v.min()) for v, _ in want) >= 0
    # and the pushes do move the counts
    assert any((v != init[f:l + 1]).any() for (v, _), (f, l) in zip(want, X.shard_ranges(E.WORLD, E.ROWS)))


@pytest.mark.parametrize("step", [0, 1, 2])
def test_negative_at_each_ring_step_closes_one_shard(oracle, step):
    calls, init = E.case_negative_at(COLS, step)
    want = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init)
    first, _ = X.shard_ranges(E.WORLD, E.ROWS)[1]
    assert want[1][1] == (E.NEG, first + 40, COLS // 2)
    assert want[0][1][0] == 0 and want[2][1][0] == 0
    # the closed shard ignored call 1; the open ones did not
    one = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls[:1], init)
    assert np.array_equal(one[1][0], want[1][0]) and not np.array_equal(one[0][0], want[0][0])
    # the later the ring step, the more adds the shard holds
    if step:
        prev = E.expected(oracle, E.WORLD, E.ROWS, COLS, E.case_negative_at(COLS, step - 1)[0], init)
        assert not np.array_equal(prev[1][0], want[1][0])


def test_dip_is_invisible_to_a_final_counter_check(oracle):
    calls, init = E.case_dip(COLS)
    total = init.astype(np.int64)
    for per_rank in calls[0]:
        for p in per_rank:
            k, v = E.decode(p, COLS)
            np.add.at(total, k, v.astype(np.int64))
    assert total.min() >= 0
    want = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init)
    first, _ = X.shard_ranges(E.WORLD, E.ROWS)[2]
    assert want[2][1] == (E.NEG, first + 11, COLS - 1) and want[2][0][11, COLS - 1] == -1
    assert want[0][1][0] == 0 and want[1][1][0] == 0


def test_two_ranks_ring_order_differs_from_rank_major(oracle):
    calls, init = E.case_two_ranks(COLS)
    ring = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init)
    major = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init, order=X.rank_major)
    first, _ = X.shard_ranges(E.WORLD, E.ROWS)[1]
    assert ring[1][1] == (E.NEG, first + 7, 0) and major[1][1] == (E.NEG, first + 300, COLS - 1)
    assert not np.array_equal(ring[1][0], major[1][0])
    # the loser's position is the smaller one
    ka, _ = E.decode(calls[0][2][2], COLS)
    kb, _ = E.decode(calls[0][0][0], COLS)
    assert (2, int(np.flatnonzero(ka == first + 7)[0])) > (0, int(np.flatnonzero(kb == first + 300)[0]))


def test_late_subchunk_holds_the_earliest_position(oracle):
    calls, init = E.case_late_subchunk(COLS)
    first, last = X.shard_ranges(E.WORLD, E.ROWS)[0]
    n = last - first + 1
    keys, _ = E.decode(calls[0][1][1], COLS)
    pos = {int(k): i for i, k in enumerate(keys)}
    bad = last - 5
    assert bad - first >= n - n // 4 and pos[bad] == 2
    quarter = [k for k in range(first, first + n // 4)]
    assert all(pos[k] > pos[bad] for k in quarter)
    want = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init)
    assert want[0][1] == (E.NEG, bad, COLS - 1)
    # those first-quarter rows hold rank 0's three pushes and rank 1's push 0 only
    part = init[first:first + n // 4].astype(np.int64)
    for p in calls[0][0] + calls[0][1][:1]:
        k, v = E.decode(p, COLS)
        m = (k >= first) & (k < first + n // 4)
        np.add.at(part, k[m] - first, v[m].astype(np.int64))
    assert np.array_equal(part.astype(E.I4), want[0][0][:n // 4])


def test_int_max_plus_one(oracle):
    calls, init = E.case_int_max(COLS)
    want = E.expected(oracle, E.WORLD, E.ROWS, COLS, calls, init)
    assert want[0][1] == (E.NEG, 3, 0) and want[0][0][3, 0] == -2 ** 31

"""CPU: the chained reduce-scatter's yardstick (tests/chain_expect.py) discriminates,
and the bindings of the chained path exist.

The GPU tests (test_gpu_chain.py, test_native_chain.py) compare every shard, byte
for byte, with the oracle fed the ring order "rank s, s+1, ..., s-1". That proves
the order only if another order gives other bytes: here the rank-major order
0..N-1 (what the exchange path applies) is shown to differ from the ring order on
the very inputs those tests use (1000 x 64, W = 3, three calls, worlds 2-4).

Measured with the oracle on these inputs, shards s != 0:
  fp32  share of elements whose bits differ  0.401 - 0.431
  fp64  count of elements whose bits differ  49 - 73 per shard (0.0023 - 0.0037)
The asserted floors (10 % of the elements; 10 elements) are under a third of those.
Shard 0's ring order is the rank-major order, so it must not differ at all.
"""
import numpy as np
import pytest

import chain_expect as X

ROWS, COLS, W, CALLS = 1000, 64, 3, 3


@pytest.mark.parametrize("vt,world", [(vt, w) for vt in (1, 3) for w in (2, 3, 4)])
def test_ring_order_differs_from_rank_major(oracle, vt, world):
    calls = X.chain_calls(oracle, vt, world, ROWS, COLS, W, CALLS)
    ring = X.expected_shards(oracle, vt, world, ROWS, COLS, calls)
    major = X.expected_shards(oracle, vt, world, ROWS, COLS, calls, order=X.rank_major)
    assert X.same_bits(ring[0], major[0], vt)  # shard 0: the same order
    for s in range(1, world):
        diff = X.bits(ring[s], vt) != X.bits(major[s], vt)
        print(f"vt {vt} world {world} shard {s}: {int(diff.sum())} of {diff.size} differ ({diff.mean():.4f})")
        if vt == 1:
            assert diff.mean() >= 0.10, (s, diff.mean())
        else:
            assert diff.sum() >= 10, (s, int(diff.sum()))
        # and both are the same sums up to rounding: the orders differ, not the pushes
        assert np.allclose(ring[s], major[s], rtol=1e-4 if vt == 1 else 1e-12, atol=1e-5 if vt == 1 else 1e-13)


def test_restrict_keeps_order_and_bytes(oracle):
    """A push restricted to every shard in turn gives back, shard by shard, the oracle
    state of the unrestricted push (the codec round-trips records byte for byte)."""
    import test_gpu_group as G
    p = G._buckets(oracle, 1, 1, 2, ROWS, COLS, 0)[1]
    whole = oracle.OracleStore(1, 0, 1, 0, ROWS - 1, COLS)
    whole.data[:] = X.init_values(1, ROWS, COLS)
    assert whole.push(p.tobytes()) == 0
    got = X.expected_shards(oracle, 1, 3, ROWS, COLS, [[[p], [], []]])
    assert X.same_bits(np.concatenate(got), whole.data, 1)
    assert sum(len(X.restrict(p, 1, COLS, f, l)) for f, l in X.shard_ranges(3, ROWS)) == p.nbytes


def test_minus_zero_is_told_apart():
    a = np.array([0.0, -0.0], np.float32)
    assert np.array_equal(a, a[::-1]) and not X.same_bits(a, a[::-1], 1)


def test_chained_symbols_are_bound():
    """The three C-ABI entry points of the chained path are declared, bound and exported,
    and the Python group exposes the call."""
    from distml_amd import _lib
    from distml_amd.group import HipOps, NativeShardGroup
    L = _lib.load()
    for name in ("dml_prereduce_chain_piece", "dml_store_assign_dense_device", "dml_group_push_chained"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert callable(NativeShardGroup.push_chained)
    assert callable(HipOps.chain_piece) and callable(HipOps.assign)

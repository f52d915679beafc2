"""GPU, multi-process: dml_group_push_chained (the order-exact chained
reduce-scatter of the native shard group) at world 1-4, in torch-free worker
processes (tests/chain_group_worker.py) over tests/rccl_double — the stand-in that
lets several ranks share one GPU and runs every transfer 20 ms after its inputs
are ready, so a stream dependency the library forgets shows up as wrong bytes.

Every shard is compared, byte for byte (unsigned view: -0.0 is not +0.0), with
tests/chain_expect.py: one oracle store per shard, fed the ring order "rank s,
s+1, ..., s-1". tests/test_chain_expect.py shows that the rank-major order gives
other bytes on these inputs, so a chain in the wrong order cannot pass.
test_native_chain_rccl_all_devices runs the same over the system RCCL where the
box has more than one GPU (skipped on one).
"""
import functools

import numpy as np
import pytest

import chain_expect as X
import group_ranks as R

pytestmark = pytest.mark.gpu
CALLS = 3


run_ranks = functools.partial(R.run_ranks, "chain_group_worker.py", no_transfers=("unsup",))


def shard_bytes(tmp_path, case, r, vt, cols):
    return np.load(tmp_path / f"{case}_{r}.npz")["data"].reshape(-1).view(X.VDT[vt]).reshape(-1, cols)


def assert_shards(tmp_path, case, world, vt, cols, want):
    for s in range(world):
        got = shard_bytes(tmp_path, case, s, vt, cols)
        assert X.same_bits(got, want[s], vt), (case, s, int((X.bits(got, vt) != X.bits(want[s], vt)).sum()))


# 1000 rows: shards of 334, 334, 332 rows at world 3 (pieces 4: sub-chunks of 84, 84, 84, 82 /
# 83 x 4), 250 at world 4; 1198 x 200 ascending: the up-front identity check and k_flat_ident;
# 100 rows, pieces 8: shards of 34, 34, 32, sub-chunks of 5 x 6, 4, 0 / 4 x 8 — an empty last
# sub-chunk is sent while a non-empty one is received, and the reverse
CHAIN_CASES = [(1, 1, 1000, 64, 1, 0), (2, 1, 1000, 64, 1, 0), (3, 1, 1000, 64, 2, 0), (4, 1, 1000, 67, 1, 0),
               (3, 1, 1000, 64, 4, 0), (3, 3, 1000, 64, 2, 0), (3, 1, 1198, 200, 1, 1), (3, 1, 100, 64, 8, 0)]


def run_chain_case(tmp_path, oracle, world, vt, rows, cols, pieces, asc, double=True):
    W = 3
    outs = run_ranks(tmp_path, world, "chain", double=double, vt=vt, rows=rows, cols=cols, pushes=W, pieces=pieces,
                     asc=asc)
    assert all(not d["errors"] for d in outs), outs
    calls = X.chain_calls(oracle, vt, world, rows, cols, W, CALLS, asc=bool(asc), short=lambda r, c: (r, c) == (0, 1))
    assert_shards(tmp_path, "chain", world, vt, cols, X.expected_shards(oracle, vt, world, rows, cols, calls))


@pytest.mark.parametrize("world,vt,rows,cols,pieces,asc", CHAIN_CASES)
def test_native_chain(tmp_path, oracle, world, vt, rows, cols, pieces, asc):
    """Three chained calls back to back without a flush (the two buffer sets rotate),
    W = 3; in call 1 rank 0 passes no push and the others three. Bytes-equal."""
    run_chain_case(tmp_path, oracle, world, vt, rows, cols, pieces, asc)


def test_native_chain_orders_with_push_local(tmp_path, oracle):
    """chained, push_local of the rank's own rows, chained — no flush in between: bytes-equal
    to the oracle in that order (fp32 adds do not commute in their roundings)."""
    world, vt, rows, cols, W = 3, 1, 1000, 64, 3
    outs = run_ranks(tmp_path, world, "order", vt=vt, rows=rows, cols=cols, pushes=W, pieces=2)
    assert all(not d["errors"] for d in outs), outs
    calls = X.chain_calls(oracle, vt, world, rows, cols, W, 2)
    rng = X.shard_ranges(world, rows)
    want = X.expected_shards(oracle, vt, world, rows, cols, calls,
                             after=lambda s, c: [X.local_push(vt, s, rng[s][0], rng[s][1], cols)] if c == 0 else [])
    assert_shards(tmp_path, "order", world, vt, cols, want)
    # the yardstick sees the order: the local push applied last gives other bytes
    late = X.expected_shards(oracle, vt, world, rows, cols, calls,
                             after=lambda s, c: [X.local_push(vt, s, rng[s][0], rng[s][1], cols)] if c == 1 else [])
    assert not X.same_bits(late[0], want[0], vt)


def test_native_chain_local_failure_keeps_the_ring(tmp_path, oracle):
    """World 3: rank 1's call 1 hands over a push one byte short. Rank 1 raises exactly
    once, at that call, with the reference's mapping for a record cut short
    (ArrayIndexOutOfBoundsException); every rank finishes every call; every shard — rank
    1's too — is bytes-equal to the ring order without rank 1's call 1. The init holds
    -0.0 in rows no push lists: a rank that added zeros instead of forwarding the slice
    would turn them into +0.0."""
    world, vt, rows, cols, W = 3, 1, 1000, 64, 3
    outs = run_ranks(tmp_path, world, "fail", vt=vt, rows=rows, cols=cols, pushes=W, pieces=2)
    assert [len(d["errors"]) for d in outs] == [0, 1, 0], outs
    assert outs[1]["errors"][0][:2] == [1, "ArrayIndexOutOfBoundsException"], outs[1]
    calls = [[X.subset_pushes(vt, r, W, rows, cols, c) for r in range(world)] for c in range(CALLS)]
    init = X.minus_zero_init(vt, rows, cols)
    want = X.expected_shards(oracle, vt, world, rows, cols, calls, init=init, skip=lambda r, c: (r, c) == (1, 1))
    assert_shards(tmp_path, "fail", world, vt, cols, want)
    neg0 = X.bits(np.array([-0.0]), vt)[0]
    for s, (f, l) in enumerate(X.shard_ranges(world, rows)):
        un = np.arange(5, rows, 7)
        un = un[(un >= f) & (un <= l)] - f
        assert (X.bits(shard_bytes(tmp_path, "fail", s, vt, cols), vt)[un] == neg0).all(), s


def test_native_chain_through_jni(tmp_path, oracle):
    """GpuShardGroup.pushChained's native call (nativeGroupPush mode 4 in
    integration/jni/dml_jni.cc) on the mock JNIEnv at world 2, the shards read back through
    nativeWriteAll: bytes-equal."""
    world, vt, rows, cols, W = 2, 1, 1000, 64, 3
    outs = run_ranks(tmp_path, world, "jni", rows=rows, cols=cols, pushes=W)
    assert all(not d["errors"] for d in outs), outs
    calls = X.chain_calls(oracle, vt, world, rows, cols, W, 2)
    assert_shards(tmp_path, "jni", world, vt, cols, X.expected_shards(oracle, vt, world, rows, cols, calls))


def test_native_chain_refuses_int32_on_every_rank(tmp_path):
    """An int32 group's push_chained returns DML_E_UNSUPPORTED (naming the exchange path) on
    every rank before any send: no rank waits for a peer, every shard keeps its values."""
    from distml_amd import _lib
    world = 2
    outs = run_ranks(tmp_path, world, "unsup", rows=1000, cols=64)
    for d in outs:
        assert len(d["errors"]) == 1 and d["errors"][0][1] == "NativeError", d
        assert d["errors"][0][2] == _lib.DML_E_UNSUPPORTED and "dml_group_push_exchange" in d["errors"][0][3], d
    for r in range(world):
        assert not np.load(tmp_path / f"unsup_{r}.npz")["data"].any()


def test_native_chain_rccl_all_devices(tmp_path, oracle):
    """The same chained calls over the system RCCL, one GPU per rank (xGMI), at world = the
    box's GPU count."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU: RCCL refuses two ranks per device (the stand-in tests cover N > 1)")
    run_chain_case(tmp_path, oracle, min(n, 8), 1, 1000, 64, 2, 0, double=False)

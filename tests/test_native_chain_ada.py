"""GPU, multi-process: dml_group_push_chained on an AdaGrad group
(FloatMatrixStoreAdaGrad) at world 1-4, in torch-free worker processes
(tests/chain_ada_group_worker.py) over tests/rccl_double — the stand-in that lets
several ranks share one GPU and runs every transfer 20 ms after its inputs are
ready, so a stream dependency the library forgets shows up as wrong bytes. It
allows one send and one receive per peer and group: an AdaGrad sub-chunk travels
as one message.

Every rank's data, delta, alpha and maxDelta are compared, byte for byte, with
tests/chain_ada_expect.py: one AdaGrad oracle store per shard, fed the ring order.
tests/test_chain_ada_expect.py shows that the yardstick tells the ring order from
rank-major on these generators' inputs.
test_native_chain_ada_rccl_all_devices runs the same over the system RCCL where the
box has more than one GPU (skipped on one).
"""
import functools

import numpy as np
import pytest

import chain_ada_expect as A
import chain_expect as X
import group_ranks as R

pytestmark = pytest.mark.gpu


run_ranks = functools.partial(R.run_ranks, "chain_ada_group_worker.py")


def assert_ranks(tmp_path, case, world, cols, want):
    for s in range(world):
        z = np.load(tmp_path / f"{case}_{s}.npz")
        for k in ("data", "delta", "alpha"):
            got = z[k].reshape(-1).view(A.F32).reshape(-1, cols)
            assert X.same_bits(got, want[s][k], A.VT), (case, s, k,
                                                        int((X.bits(got, A.VT) != X.bits(want[s][k], A.VT)).sum()))
        md = z["md"]
        assert A.same_md((np.float32(md[0]), int(md[1]), int(md[2])), want[s]["md"]), (case, s, md, want[s]["md"])


# 1198 x 200 ascending: the vector stream; 1000 x 64 permuted: the slot-table shape. 1000 rows:
# shards of 334, 334, 332 at world 3 (a short last shard; pieces 3: sub-chunks of 112, 112, 110 /
# 111, 111, 110), 250 at world 4; 1198 rows: 400, 400, 398 at world 3; 100 rows, pieces 8: shards
# of 34, 34, 32, sub-chunks of 5 x 6, 4, 0 / 4 x 8 — the 34-row slices' maxDelta record travels on
# an empty last sub-chunk, sent while a non-empty one is received, and the reverse
CHAIN_CASES = [(1, 1000, 64, 1, 0), (2, 1198, 200, 3, 1), (3, 1000, 64, 3, 0), (3, 1198, 200, 1, 1),
               (4, 1000, 64, 1, 0), (4, 1198, 200, 3, 1), (3, 100, 64, 8, 0), (3, 100, 200, 8, 1)]


def run_chain_case(tmp_path, oracle, world, rows, cols, pieces, asc, double=True):
    outs = run_ranks(tmp_path, world, "chain", double=double, rows=rows, cols=cols, pieces=pieces, asc=asc)
    assert all(not d["errors"] for d in outs), outs
    calls = A.group_calls(world, rows, cols, bool(asc))
    want = A.expected(oracle, world, rows, cols, calls, X.init_values(A.VT, rows, cols), set_alpha={0: A.SET_ALPHA})
    assert_ranks(tmp_path, "chain", world, cols, want[-1])


@pytest.mark.parametrize("world,rows,cols,pieces,asc", CHAIN_CASES)
def test_native_chain_ada(tmp_path, oracle, world, rows, cols, pieces, asc):
    """Three chained calls back to back without a flush (the two buffer sets rotate), W = 3; in
    call 1 rank 0 passes no push; setAlpha on every store after call 0. Byte-equal."""
    run_chain_case(tmp_path, oracle, world, rows, cols, pieces, asc)


@pytest.mark.parametrize("cols,asc,rows", [(64, 0, 1000), (200, 1, 1198)])
def test_native_chain_ada_orders_with_other_calls(tmp_path, oracle, cols, asc, rows):
    """chained, push_local of the rank's own rows, push_exchange (rank-major), chained — no
    flush in between: byte-equal to the oracle in that order."""
    world = 3
    outs = run_ranks(tmp_path, world, "order", rows=rows, cols=cols, pieces=3, asc=asc)
    assert all(not d["errors"] for d in outs), outs
    calls = A.calls(world, A.GROUP_W, rows, cols, A.GROUP_CALLS, asc=bool(asc))
    rng = X.shard_ranges(world, rows)
    adds = world * A.GROUP_W * A.GROUP_CALLS
    init = X.init_values(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init, orders={1: X.rank_major},
                      after=lambda s, c: [A.local_push(s, rng[s][0], rng[s][1], cols, adds)] if c == 0 else [])
    assert_ranks(tmp_path, "order", world, cols, want[-1])
    # the yardstick sees the order: the exchange call in ring order gives other delta bits
    other = A.expected(oracle, world, rows, cols, calls, init,
                       after=lambda s, c: [A.local_push(s, rng[s][0], rng[s][1], cols, adds)] if c == 0 else [])
    assert not X.same_bits(other[-1][1]["delta"], want[-1][1]["delta"], A.VT)


def test_native_chain_ada_local_failure_keeps_the_ring(tmp_path, oracle):
    """World 3: rank 1's call 1 hands over a push one byte short. Rank 1 raises exactly once, at
    that call (ArrayIndexOutOfBoundsException); every rank finishes every call; every shard is
    byte-equal to the ring order without rank 1's call 1 — its pushes appear nowhere, it marked
    no row (alpha) and changed no maxDelta record. The init holds -0.0 in rows no push lists."""
    world, rows, cols = 3, 1000, 64
    outs = run_ranks(tmp_path, world, "fail", rows=rows, cols=cols, pieces=3)
    assert [len(d["errors"]) for d in outs] == [0, 1, 0], outs
    assert outs[1]["errors"][0][:2] == [1, "ArrayIndexOutOfBoundsException"], outs[1]
    calls = A.fail_calls(world, rows, cols)
    init = X.minus_zero_init(A.VT, rows, cols)
    want = A.expected(oracle, world, rows, cols, calls, init, skip=lambda r, c: (r, c) == (1, 1))
    assert_ranks(tmp_path, "fail", world, cols, want[-1])
    neg0 = X.bits(np.array([-0.0]), A.VT)[0]
    for s, (f, l) in enumerate(X.shard_ranges(world, rows)):
        un = np.arange(5, rows, 7)
        un = un[(un >= f) & (un <= l)] - f
        got = np.load(tmp_path / f"fail_{s}.npz")["data"].reshape(-1).view(A.F32).reshape(-1, cols)
        assert (X.bits(got, A.VT)[un] == neg0).all(), s


def test_native_chain_ada_through_jni(tmp_path, oracle):
    """GpuShardGroup.pushChained's native call (nativeGroupPush mode 4) on the mock JNIEnv with
    an AdaGrad group at world 2; data read back through nativeWriteAll, alpha and delta through
    nativeSnapshot, maxDelta through nativeMaxDelta: byte-equal."""
    world, rows, cols = 2, 1000, 64
    outs = run_ranks(tmp_path, world, "jni", rows=rows, cols=cols, pieces=2)
    assert all(not d["errors"] for d in outs), outs
    calls = A.group_calls(world, rows, cols, False)[:2]
    want = A.expected(oracle, world, rows, cols, calls, X.init_values(A.VT, rows, cols))
    assert_ranks(tmp_path, "jni", world, cols, want[-1])


def test_native_chain_ada_rccl_all_devices(tmp_path, oracle):
    """The same chained calls over the system RCCL, one GPU per rank (xGMI), at world = the
    box's GPU count."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU: RCCL refuses two ranks per device (the stand-in tests cover N > 1)")
    run_chain_case(tmp_path, oracle, min(n, 8), 1198, 200, 3, 1, double=False)

"""GPU, multi-process: dml_group_push_chained_i32 (IntMatrixStore groups) at world
2-4, in torch-free worker processes (tests/chain_i32_group_worker.py) over
tests/rccl_double — the stand-in that lets several ranks share one GPU and runs every
transfer 20 ms after its inputs are ready, so a stream dependency the library forgets
shows up as wrong bytes. It allows one send and one receive per peer and group: the
verdict record rides inside sub-chunk 0's message.

Every rank's shard and error state are compared with tests/chain_i32_expect.py: one
int32 oracle store per shard, fed the ring order and stopped at its first negative.
test_native_chain_i32_rccl_all_devices runs the clean case over the system RCCL where
the box has more than one GPU (skipped on one).
"""
import functools

import numpy as np
import pytest

import chain_expect as X
import chain_i32_expect as E
import group_ranks as R

pytestmark = pytest.mark.gpu
ISE, AIOOBE = "IllegalStateException", "ArrayIndexOutOfBoundsException"


run_ranks = functools.partial(R.run_ranks, "chain_i32_group_worker.py", no_transfers=("refuse",))


def assert_ranks(tmp_path, case, world, cols, want):
    for s in range(world):
        z = np.load(tmp_path / f"{case}_{s}.npz")
        got = z["data"].reshape(-1).view(E.I4).reshape(-1, cols)
        assert got.tobytes() == want[s][0].tobytes(), (case, s, int((got != want[s][0]).sum()))
        assert tuple(int(v) for v in z["state"]) == want[s][1], (case, s, z["state"], want[s][1])


def assert_only_owner_reports(outs, owner, want, first_where=None):
    """The owner of the closed shard raises the IllegalStateException with the oracle's key and
    col, at least once (its next call, or the flush); nobody else raises anything."""
    for r, d in enumerate(outs):
        if r != owner:
            assert not d["errors"], (r, d)
    errs = outs[owner]["errors"]
    assert errs and all(e[1] == ISE and (e[2], e[3]) == want[owner][1][1:] for e in errs), errs
    if first_where is not None:
        assert errs[0][0] == first_where, errs


# 1000 rows: shards of 500 at world 2; 334, 334, 332 at world 3 (pieces 2: sub-chunks of 167 / 166);
# 250 at world 4. 67 columns: pair-packed k_reduce_rows; 256: FULL; 3: k_reduce. 100 rows, pieces 8:
# shards of 34, 34, 32 in sub-chunks of 5 x 6, 4, 0 / 4 x 8 — a step skips the piece of an empty
# sub-chunk, and an empty last sub-chunk is sent while a non-empty one is received, and the reverse
# (the adds commute and init >= 1000 keeps every count positive: this pins the plumbing, not the order)
CHAIN_CASES = [(2, 67, 1, 1000), (3, 67, 2, 1000), (4, 256, 2, 1000), (3, 3, 1, 1000), (3, 67, 8, 100)]
CHAIN_IDS = ["-".join(map(str, c if c[3] != 1000 else c[:3])) for c in CHAIN_CASES]


def run_chain_case(tmp_path, oracle, world, cols, pieces, double=True, rows=1000):
    outs = run_ranks(tmp_path, world, "chain", double=double, rows=rows, cols=cols, pieces=pieces)
    assert all(not d["errors"] for d in outs), outs
    want = E.expected(oracle, world, rows, cols, E.group_calls(world, rows, cols, "chain"), E.init_counts(rows, cols))
    assert all(w[1][0] == 0 for w in want)
    assert_ranks(tmp_path, "chain", world, cols, want)


@pytest.mark.parametrize("world,cols,pieces,rows", CHAIN_CASES, ids=CHAIN_IDS)
def test_native_chain_i32(tmp_path, oracle, world, cols, pieces, rows):
    """Three clean chained calls back to back without a flush (the two buffer sets rotate),
    W = 3; in call 1 rank 0 passes no push. Byte-equal, no error anywhere."""
    run_chain_case(tmp_path, oracle, world, cols, pieces, rows=rows)


@pytest.mark.parametrize("world,cols,pieces", [(2, 67, 2), (3, 1000, 2), (4, 67, 1)])
def test_native_chain_i32_closed_shard_stays_frozen(tmp_path, oracle, world, cols, pieces):
    """Call 0 closes shard 1 at the rank after its owner; two more chained calls follow with no
    flush. Shard 1 holds the adds up to the failing one and nothing of calls 1 and 2; its owner's
    next call or flush raises with the oracle's key and col; the other shards go on."""
    rows = 1000
    outs = run_ranks(tmp_path, world, "close", rows=rows, cols=cols, pieces=pieces)
    want = E.expected(oracle, world, rows, cols, E.group_calls(world, rows, cols, "close"), E.init_counts(rows, cols))
    assert [w[1][0] for w in want] == [E.NEG if s == 1 else 0 for s in range(world)]
    assert_only_owner_reports(outs, 1, want)
    assert_ranks(tmp_path, "close", world, cols, want)


def test_native_chain_i32_orders_with_other_calls(tmp_path, oracle):
    """chained (rank 1's own push closes its own shard), push_local, push_exchange, chained — no
    flush. Rank 1's push_local waits for the commit's verdict and is refused, as the reference's
    server refuses every push after the exception; nothing later reaches shard 1. The other
    shards take all four calls in order (the exchange call rank-major)."""
    world, rows, cols = 3, 1000, 67
    outs = run_ranks(tmp_path, world, "order", rows=rows, cols=cols, pieces=2)
    rng = X.shard_ranges(world, rows)
    want = E.expected(oracle, world, rows, cols, E.group_calls(world, rows, cols, "order"), E.init_counts(rows, cols),
                      orders={1: X.rank_major},
                      after=lambda s, c: [E.local_push(s, rng[s][0], rng[s][1], cols)] if c == 0 else [])
    assert [w[1][0] for w in want] == [0, E.NEG, 0]
    assert_only_owner_reports(outs, 1, want, first_where="local")
    assert_ranks(tmp_path, "order", world, cols, want)


def test_native_chain_i32_truncated_push_beside_a_negative(tmp_path, oracle):
    """World 3, call 0: rank 2 hands over a push one byte short (it raises there, forwards every
    slice and record unchanged, its pushes reach no shard) while rank 1's push closes shard 0."""
    world, rows, cols = 3, 1000, 67
    outs = run_ranks(tmp_path, world, "fail", rows=rows, cols=cols, pieces=2)
    want = E.expected(oracle, world, rows, cols, E.group_calls(world, rows, cols, "fail"), E.init_counts(rows, cols),
                      skip=lambda r, c: (r, c) == (2, 0))
    assert [w[1][0] for w in want] == [E.NEG, 0, 0]
    assert not outs[1]["errors"], outs[1]
    assert [e[:2] for e in outs[2]["errors"]] == [[0, AIOOBE]], outs[2]
    e0 = outs[0]["errors"]
    assert e0 and all(e[1] == ISE and (e[2], e[3]) == want[0][1][1:] for e in e0), e0
    assert_ranks(tmp_path, "fail", world, cols, want)


def test_native_chain_i32_through_jni(tmp_path, oracle):
    """GpuShardGroup.pushChainedChecked's native call (nativeGroupPush mode 5) on the mock
    JNIEnv at world 2; data read back through nativeWriteAll."""
    world, rows, cols = 2, 1000, 67
    outs = run_ranks(tmp_path, world, "jni", rows=rows, cols=cols, pieces=2)
    assert all(not d["errors"] for d in outs), outs
    calls = E.group_calls(world, rows, cols, "chain")[:2]
    assert_ranks(tmp_path, "jni", world, cols, E.expected(oracle, world, rows, cols, calls, E.init_counts(rows, cols)))


def test_native_chain_i32_refuses_an_fp32_group(tmp_path):
    """DML_E_UNSUPPORTED on every rank alike, before any send; the shards are untouched."""
    from distml_amd import _lib
    world, rows, cols = 2, 1000, 64
    outs = run_ranks(tmp_path, world, "refuse", rows=rows, cols=cols)
    init = X.init_values(1, rows, cols)
    for r, (f, l) in enumerate(X.shard_ranges(world, rows)):
        assert [e[:3] for e in outs[r]["errors"]] == [[0, "NativeError", _lib.DML_E_UNSUPPORTED]], outs[r]
        assert "dml_group_push_chained" in outs[r]["errors"][0][4]
        got = np.load(tmp_path / f"refuse_{r}.npz")["data"].reshape(-1).view("<f4").reshape(-1, cols)
        assert X.same_bits(got, init[f:l + 1], 1), r


def test_native_chain_i32_rccl_all_devices(tmp_path, oracle):
    """The clean chained calls over the system RCCL, one GPU per rank (xGMI), at world = the
    box's GPU count."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU: RCCL refuses two ranks per device (the stand-in tests cover N > 1)")
    run_chain_case(tmp_path, oracle, min(n, 8), 1000, 2, double=False)

"""GPU, multi-process: the collective group pull (dml_group_pull, NativeShardGroup.pull) in
torch-free worker processes (tests/pull_group_worker.py). World 2-4 shares one GPU over
tests/rccl_double, which runs every transfer 20 ms after its inputs are ready, so a stream
dependency the library forgets shows up as wrong bytes; world 1 runs on the system RCCL.

Every rank's bytes, *out_len and out_counts, in both output orders, are compared with
tests/pull_expect.py (one oracle store per shard, fed in the documented order of each push
path; pinned on the CPU by tests/test_pull_expect.py). Every output sits 4 bytes past a
16-byte boundary between guard bands, with cap == *out_len exactly.

The group has no store flags, so FloatArrayStore runs at the library's default push stride
only (its fetched record has the 8-byte slot under either flag, tests/test_gpu_fetch_device.py).
"""
import functools
import time

import numpy as np
import pytest

import pull_expect as P
import group_ranks as R

pytestmark = pytest.mark.gpu

run_ranks = functools.partial(R.run_ranks, "pull_group_worker.py")


def check_pulls(tmp_path, case, world, want_by_pull, skip=()):
    """want_by_pull[i][rank] = (owner-major, request-order, counts); pull 2i is owner-major,
    pull 2i + 1 request-order. skip: ranks whose pulls are checked by the caller."""
    for r in range(world):
        if r in skip:
            continue
        z = np.load(tmp_path / f"{case}_{r}.npz")
        for i, want in enumerate(want_by_pull):
            om, rq, counts = want[r]
            for j, wb in ((2 * i, om), (2 * i + 1, rq)):
                what = (case, "rank", r, "pull", j)
                assert z[f"s{j}"].tolist() == [0, len(wb)], what
                assert z[f"c{j}"].tolist() == counts, what
                got = z[f"b{j}"].tobytes()
                if got != wb:
                    bad = np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(wb, np.uint8))
                    raise AssertionError((what, "first differing byte", int(bad[0]), "of", len(wb), "count", bad.size))
                assert bool(z[f"g{j}"]), what


@pytest.mark.parametrize("tag,world", P.TABLE, ids=[f"{t}-w{w}" for t, w in P.TABLE])
def test_native_pull_table(tmp_path, oracle, tag, world):
    """Every store of the table: f32 at 67 / 256 columns and 768 columns behind long keys (the
    16-byte-load side of k_fetch_vec), AdaGrad after a push that moved alpha (no flush before the
    pull), int32, f64, the three array stores. Per-rank key lists: every shard's first and last
    key, descending, repeats, -1 / total_rows / 2^40, own shard only, one remote shard only,
    no key; lengths 1, 257, 700."""
    case = f"table-{tag}"
    outs = run_ranks(tmp_path, world, case, double=world > 1)
    assert all(not d["errors"] for d in outs), outs
    check_pulls(tmp_path, case, world, [P.table_expected(oracle, tag, world)])


@pytest.mark.parametrize("case", sorted(P.ORDER))
def test_native_pull_orders_with_pushes(tmp_path, oracle, case):
    """push, pull, push, pull with no flush: the first pulls hold exactly the first push's state,
    the second both. push_exchange (caller stream, no synchronisation between the calls: ord_x),
    push_chained fp32 and AdaGrad, push_chained_i32 + push_local."""
    tag, world, _ = P.ORDER[case]
    outs = run_ranks(tmp_path, world, case, pieces=2 if case != "ord_x" else 1)
    assert all(not d["errors"] for d in outs), outs
    check_pulls(tmp_path, case, world, P.order_expected(oracle, case))


def test_native_pull_closed_int32_shard_answers(tmp_path, oracle):
    """chain_i32_expect's "close" call closes shard 1; after the flush reported it to its owner, a
    pull returns DML_OK on every rank and shard 1's rows are the frozen state."""
    tag, world = P.CLOSED
    outs = run_ranks(tmp_path, world, "closed", pieces=2)
    for r, d in enumerate(outs):
        if r == 1:
            assert d["errors"] and all(e[1] == "IllegalStateException" for e in d["errors"]), d
        else:
            assert not d["errors"], d
    check_pulls(tmp_path, "closed", world, [P.closed_expected(oracle)])
    assert int(np.load(tmp_path / "closed_1.npz")["state"][0]) == 4  # DML_E_NEGATIVE_COUNTER, still sticky


def test_native_pull_short_cap_strands_nobody(tmp_path, oracle):
    """Rank 1's cap is one byte short: it gets DML_E_CAPACITY (with the length and counts it
    needed), writes nothing, and every other rank gets its bytes — well inside the harness's
    240 s limit, which a rank waiting for another would run into."""
    from distml_amd import _lib
    tag, world = "f32c67", 3
    t0 = time.time()
    outs = run_ranks(tmp_path, world, "cap")
    assert time.time() - t0 < 120
    assert all(not d["errors"] for d in outs), outs
    want = P.table_expected(oracle, tag, world)
    check_pulls(tmp_path, "cap", world, [want], skip=(1,))
    z = np.load(tmp_path / "cap_1.npz")
    for j in (0, 1):
        assert z[f"s{j}"].tolist() == [_lib.DML_E_CAPACITY, len(want[1][0])]
        assert z[f"c{j}"].tolist() == want[1][2]
        assert bool(z[f"g{j}"])  # nothing written: not into the output, not past the guards
        assert (z[f"b{j}"].view("<u4") == 0x7FF7FFFF).all()


def test_native_pull_through_jni(tmp_path, oracle):
    """GpuShardGroup.pull's native call (nativeGroupPull) on the mock JNIEnv at world 2, both
    output orders; the counts come back as little-endian int64 in a byte[]."""
    tag, world = "f32c67", 2
    outs = run_ranks(tmp_path, world, "jni")
    assert all(not d["errors"] for d in outs), outs
    check_pulls(tmp_path, "jni", world, [P.table_expected(oracle, tag, world)])


def test_native_pull_rccl_all_devices(tmp_path, oracle):
    """The f32 table case over the system RCCL, one GPU per rank (xGMI), at world = the box's
    GPU count, at most 8."""
    import torch
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("one GPU: RCCL refuses two ranks per device (the stand-in tests cover N > 1)")
    world = min(n, 8)
    outs = run_ranks(tmp_path, world, "table-f32c67", double=False)
    assert all(not d["errors"] for d in outs), outs
    check_pulls(tmp_path, "table-f32c67", world, [P.table_expected(oracle, "f32c67", world)])

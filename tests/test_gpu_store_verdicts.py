"""GPU, one process: the store's sticky device verdicts across dml_store_clear_error.

An int32 owner apply (dml_store_apply_dense_device) and a chained int32 commit
(dml_store_assign_dense_i32_device) each keep a sticky record in HBM that is mirrored to the
host behind the call. Once reported, the record stays closed until clear_error reopens it:
after that a clean call passes and a new failure is reported with its own key and column,
not the first one's. (The device list fetch's verdict, which reopens itself when it is
reported, is covered by tests/test_gpu_fetch_device.py.)
"""
import struct

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS, COLS, FIRST = 64, 8, 100
NEG = 4  # DML_E_NEGATIVE_COUNTER
OPEN = b"\xff" * 32


def _store():
    from distml_amd import DataDesc, DataStore, KeyRange
    st = DataStore(DataDesc(1, 0, 0), KeyRange(FIRST, FIRST + ROWS - 1), COLS, async_push=True)
    st.fill(3)
    return st


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _raises_at(call, key, col):
    from distml_amd.store import IllegalStateException
    with pytest.raises(IllegalStateException) as ei:
        call()
    assert (ei.value.code, ei.value.key, ei.value.col) == (NEG, key, col)


def test_owner_apply_verdict_reopens_at_clear_error():
    from distml_amd.group import HipOps
    ops, st = HipOps(), _store()
    n = ROWS * COLS
    want = np.full((ROWS, COLS), 3, np.int32)
    zero = _dev(np.zeros(n, np.int32))

    def delta(r, c):
        d = np.zeros((ROWS, COLS), np.int32)
        d[r, c] = -4
        return _dev(d.reshape(-1))

    d1, d2 = delta(5, 2), delta(41, 7)
    ops.apply(st, d1.data_ptr(), n)
    _raises_at(st.flush, FIRST + 5, 2)
    assert st.error_state() == (NEG, FIRST + 5, 2)
    _raises_at(lambda: ops.apply(st, zero.data_ptr(), n), FIRST + 5, 2)  # refused: the sticky state
    st.clear_error()
    assert st.error_state()[0] == 0
    # the failing apply's sums stay in the shard, as IntMatrixStore leaves them: the check is on
    # the final counters, so the element that is still negative is found again
    want[5, 2] = -1
    assert st.values().tobytes() == want.tobytes()
    ops.apply(st, zero.data_ptr(), n)
    _raises_at(st.flush, FIRST + 5, 2)
    st.clear_error()
    # repaired, the reopened record lets a clean apply pass
    st.fill(3)
    want[5, 2] = 3
    ops.apply(st, zero.data_ptr(), n)
    st.flush()
    assert st.error_state()[0] == 0 and st.values().tobytes() == want.tobytes()
    # and a new failure is its own element, not the first one's
    ops.apply(st, d2.data_ptr(), n)
    _raises_at(st.flush, FIRST + 41, 7)
    assert st.error_state() == (NEG, FIRST + 41, 7)
    want[41, 7] = -1
    assert st.values().tobytes() == want.tobytes()
    st.close()


def test_chained_commit_verdict_reopens_at_clear_error():
    from distml_amd.group import HipOps
    ops, st = HipOps(), _store()
    n = ROWS * COLS

    def closed(key, col):  # ChainI32Rec: [u64 pos][i64 key][i32 col][i32 ring step][u64 pad]
        return _dev(np.frombuffer(struct.pack("<QqiIQ", (1 << 40) | 12, key, col, 1, 0), np.uint8))

    srcs = [np.arange(n, dtype=np.int32).reshape(ROWS, COLS) + 10 * i for i in range(4)]
    dsrc = [_dev(a.reshape(-1)) for a in srcs]
    k1, c1, k2, c2 = FIRST + 9, 3, FIRST + 60, 6
    rec1, rec2, rec_open = closed(k1, c1), closed(k2, c2), _dev(np.frombuffer(OPEN, np.uint8))

    ops.assign_i32(st, dsrc[0].data_ptr(), n, rec1.data_ptr())
    _raises_at(st.flush, k1, c1)
    assert st.values().tobytes() == srcs[0].tobytes()
    # reported and not cleared: calls are refused, and the first verdict stays the state
    _raises_at(lambda: ops.assign_i32(st, dsrc[1].data_ptr(), n, rec2.data_ptr()), k1, c1)
    assert st.error_state() == (NEG, k1, c1)
    assert st.values().tobytes() == srcs[0].tobytes()
    st.clear_error()
    assert st.error_state()[0] == 0
    ops.assign_i32(st, dsrc[2].data_ptr(), n, rec_open.data_ptr())
    st.flush()
    assert st.error_state()[0] == 0 and st.values().tobytes() == srcs[2].tobytes()
    ops.assign_i32(st, dsrc[3].data_ptr(), n, rec2.data_ptr())
    _raises_at(st.flush, k2, c2)
    assert st.error_state() == (NEG, k2, c2)
    assert st.values().tobytes() == srcs[3].tobytes()
    st.close()

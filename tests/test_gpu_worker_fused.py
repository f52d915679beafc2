"""The repeats worker of tests/test_gpu_worker_coalesce.py on the fused calls, against the host worker on a
twin store: keys-only run -> handleFetchDevice -> expand_fetch_device -> gradient -> run_packed -> pushDevice."""
import numpy as np
import pytest

from test_gpu_worker_coalesce import _gpu, host_accumulate  # noqa: F401  (_gpu: the module's GPU gate)
import codec_cases as cc
from test_gpu_worker_iteration import KINDS, host_fetch, make_store

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c["id"])
def test_fused_worker_iteration_with_repeats(case):
    """900 occurrences of 301 rows; three iterations on one stream."""
    from distml_amd import Coalescer, DeviceKeys, encode_matrix_push, expand_fetch_device, record_bytes
    rows, cols, first = case["rows"], case["cols"], case["first"]
    rng = np.random.default_rng(47)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    A, B = make_store(case, init), make_store(case, init)
    fmt = A.format
    push_rec, fetch_rec = record_bytes(fmt, cols)
    co, st, n = Coalescer(0), torch.cuda.Stream(), 900
    try:
        for it in range(3):
            pool = first + rng.permutation(rows)[:301].astype(np.int64)
            keys = pool[rng.integers(0, 301, size=n)]
            dk = torch.from_numpy(keys.copy()).cuda()
            ukeys = torch.empty(n, dtype=torch.int64, device="cuda")
            inv = torch.empty(n, dtype=torch.int32, device="cuda")
            fetched = torch.empty(n * fetch_rec // 4 + 1, dtype=torch.int32, device="cuda")[1:]  # 4 mod 16
            occ = torch.empty((n, cols), dtype=torch.float32, device="cuda")
            alpha = torch.empty((n, cols), dtype=torch.float32, device="cuda") if case["ada"] else None
            packed = torch.empty(n * push_rec // 4 + 3, dtype=torch.int32, device="cuda")[3:]    # 12 mod 16
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                m = co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), None, ukeys.data_ptr(), None, inv.data_ptr(), n,
                           stream=st.cuda_stream)
                assert A.handleFetchDevice(fmt, DeviceKeys(ukeys.data_ptr(), m), fetched.data_ptr(), m * fetch_rec,
                                           stream=st.cuda_stream) == m * fetch_rec
                expand_fetch_device(fmt, cols, fetched.data_ptr(), m, inv.data_ptr(), n, occ.data_ptr(),
                                    alpha.data_ptr() if case["ada"] else None, stream=st.cuda_stream)
                grad = (occ * -0.125 + (torch.arange(n, device="cuda") * 0.001 + (it + 1) * 0.0625)[:, None]).contiguous()
                assert co.run_packed(fmt, cols, DeviceKeys(dk.data_ptr(), n), grad.data_ptr(), packed.data_ptr(),
                                     m * push_rec, stream=st.cuda_stream) == (m, m * push_rec)
            st.synchronize()  # a push reads its buffers from the store's own streams
            A.pushDevice([packed.data_ptr()], [m * push_rec])
            hinv = inv.cpu().numpy()  # the host worker's gradient is the device's: the expand is checked here
            _, hv, ha = cc.unpack_expected(case, host_fetch(B, np.unique(keys)))
            assert occ.cpu().numpy().tobytes() == hv[hinv].tobytes()
            assert not case["ada"] or alpha.cpu().numpy().tobytes() == ha[hinv].tobytes()
            sk, sv = host_accumulate(keys, grad.cpu().numpy())
            host_push = encode_matrix_push(sk, sv, case["kt"], case["vt"])
            assert packed[:m * push_rec // 4].cpu().numpy().tobytes() == host_push
            B.handlePush(fmt, host_push)
            A.flush()
            B.flush()
            assert A.values().tobytes() == B.values().tobytes(), it
            assert not case["ada"] or all(x.tobytes() == y.tobytes()
                                          for x, y in zip(A.adagrad_state(), B.adagrad_state())), it
    finally:
        for x in (co, A, B):
            x.close()

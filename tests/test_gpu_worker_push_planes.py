"""The worker of tests/test_gpu_worker_planes.py with its push half replaced as well, against the host
worker on a twin store: handleFetchPlanesDevice -> gradient -> handlePushPlanesDevice, all on one side
stream with no synchronize between them."""
import numpy as np
import pytest

from test_gpu_worker_coalesce import _gpu, host_accumulate  # noqa: F401  (_gpu: the module's GPU gate)
import codec_cases as cc
from test_gpu_worker_iteration import KINDS, host_fetch, make_store

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c["id"])
def test_record_free_worker_iteration(case):
    """900 occurrences of 301 rows; three iterations; values and AdaGrad state byte-equal to the host worker's."""
    from distml_amd import Coalescer, DeviceKeys, encode_matrix_push
    rows, cols, first, rng = case["rows"], case["cols"], case["first"], np.random.default_rng(47)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    A, B = make_store(case, init), make_store(case, init)
    fmt, co, st, n = A.format, Coalescer(0), torch.cuda.Stream(), 900
    try:
        for it in range(3):
            pool = first + rng.permutation(rows)[:301].astype(np.int64)
            keys = pool[rng.integers(0, 301, size=n)]
            dk = torch.from_numpy(keys.copy()).cuda()
            occ = torch.empty(n * cols + 1, dtype=torch.float32, device="cuda")[1:].view(n, cols)    # 4 mod 16
            alpha = torch.empty(n * cols + 3, dtype=torch.float32, device="cuda")[3:].view(n, cols) if case["ada"] else None
            gbuf = torch.empty(n * cols + 3, dtype=torch.float32, device="cuda")[3:].view(n, cols)   # 12 mod 16
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                A.handleFetchPlanesDevice(fmt, DeviceKeys(dk.data_ptr(), n), occ.data_ptr(),
                                          alpha.data_ptr() if case["ada"] else None, stream=st.cuda_stream)
                gbuf.copy_(occ * -0.125 + (torch.arange(n, device="cuda") * 0.001 + (it + 1) * 0.0625)[:, None])
                A.handlePushPlanesDevice(fmt, co, DeviceKeys(dk.data_ptr(), n), gbuf.data_ptr(), stream=st.cuda_stream)
            _, hv, ha = cc.unpack_expected(case, host_fetch(B, keys))  # the host worker's rows, per occurrence
            A.flush()
            assert occ.cpu().numpy().tobytes() == hv.tobytes()
            assert not case["ada"] or alpha.cpu().numpy().tobytes() == ha.tobytes()
            B.handlePush(fmt, encode_matrix_push(*host_accumulate(keys, gbuf.cpu().numpy()), case["kt"], case["vt"]))
            B.flush()
            assert A.values().tobytes() == B.values().tobytes(), it
            assert not case["ada"] or all(x.tobytes() == y.tobytes()
                                          for x, y in zip(A.adagrad_state(), B.adagrad_state())), it
            assert not case["ada"] or A.maxDelta() == B.maxDelta(), it
    finally:
        for x in (co, A, B):
            x.close()

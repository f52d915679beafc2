"""A worker that never leaves HBM against the same worker on the host path.

Two stores of each kind hold identical contents. Store A's worker runs handleFetchDevice ->
unpack_fetch_device -> an elementwise torch update of the values -> pack_push_device ->
synchronise -> pushDevice; store B's worker gets the same gradient through
handlePush(encode_matrix_push(keys, grad.cpu())). After each of three iterations the two
stores are byte-equal (AdaGrad: values and both state planes), and the planes A's worker
unpacked equal the numpy decode of B's handleFetch.
"""
import numpy as np
import pytest

import codec_cases as cc
import fetch_cases as fc
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# f32 at 50 columns behind int32 keys: 204-byte records, 12 mod 16; AdaGrad at 200 columns, long keys
KINDS = [fc._case("f32", 1, 0, 1, 50, 1237, geom.NEG32), fc._case("ada", 1, 1, 1, 200, 1237, geom.BIG33, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def make_store(case, init):
    from distml_amd import DataDesc, DataStore, KeyRange
    fmt = DataDesc(case["dt"], case["kt"], case["vt"], False, True, case["ada"])
    s = DataStore(fmt, KeyRange(case["first"], case["first"] + case["rows"] - 1), case["cols"])
    if case["ada"]:
        s.setAlpha(*fc.ADA)
    s.load_values(init)
    return s


def host_fetch(s, keys):
    """handleFetch of a host key list as given, repeats included (a KeyList holds a key once)."""
    import ctypes as C
    from distml_amd import _lib
    cap = len(keys) * s._fetch_record_bytes()
    out, ln = np.empty(cap, np.uint8), C.c_int64()
    assert _lib.load().dml_store_fetch(s._h, keys.ctypes.data_as(C.POINTER(C.c_int64)), len(keys), out.ctypes.data,
                                       cap, C.byref(ln)) == 0 and ln.value == cap
    return out.tobytes()


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c["id"])
def test_device_worker_equals_host_worker(case):
    from distml_amd import DeviceKeys, encode_matrix_push, pack_push_device, record_bytes, unpack_fetch_device
    rows, cols, first = case["rows"], case["cols"], case["first"]
    rng = np.random.default_rng(31)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    A, B = make_store(case, init), make_store(case, init)
    fmt = A.format
    push_rec, fetch_rec = record_bytes(fmt, cols)
    assert (push_rec, fetch_rec) == (cc.push_record_bytes(case), fc.record_bytes(case))
    assert case["ada"] or push_rec == 204
    st = torch.cuda.Stream()
    try:
        for it in range(3):
            # a key list with a repeat: the fetch returns the row twice, the push adds to it twice
            r = rng.permutation(rows)[:301]
            r[17] = r[200]
            keys = first + r.astype(np.int64)
            n = len(keys)
            dk = torch.from_numpy(keys.copy()).cuda()
            fetched = torch.empty(n * fetch_rec // 4 + 1, dtype=torch.int32, device="cuda")[1:]  # 4 mod 16
            vals = torch.empty((n, cols), dtype=torch.float32, device="cuda")
            alpha = torch.empty((n, cols), dtype=torch.float32, device="cuda") if case["ada"] else None
            kout = torch.empty(n, dtype=torch.int64, device="cuda")
            packed = torch.empty(n * push_rec // 4 + 3, dtype=torch.int32, device="cuda")[3:]    # 12 mod 16
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                assert A.handleFetchDevice(fmt, DeviceKeys(dk.data_ptr(), n), fetched.data_ptr(), n * fetch_rec,
                                           stream=st.cuda_stream) == n * fetch_rec
                unpack_fetch_device(fmt, cols, fetched.data_ptr(), n, vals.data_ptr(),
                                    alpha.data_ptr() if case["ada"] else None, kout.data_ptr(), stream=st.cuda_stream)
                grad = (vals * -0.125 + (it + 1) * 0.0625).contiguous()  # the worker's elementwise update
                assert pack_push_device(fmt, cols, DeviceKeys(kout.data_ptr(), n), grad.data_ptr(), n,
                                        packed.data_ptr(), n * push_rec, stream=st.cuda_stream) == n * push_rec
            st.synchronize()  # a push reads its buffers from the store's own streams
            A.pushDevice([packed.data_ptr()], [n * push_rec])
            # the host worker: the same fetch, decoded by numpy, and the same gradient through the host encoder
            hk, hv, ha = cc.unpack_expected(case, host_fetch(B, keys))
            assert kout.cpu().numpy().tobytes() == hk.tobytes() == keys.tobytes()
            assert vals.cpu().numpy().tobytes() == hv.tobytes()
            if case["ada"]:
                assert alpha.cpu().numpy().tobytes() == ha.tobytes()
            g = grad.cpu().numpy()
            host_push = encode_matrix_push(keys, g, case["kt"], case["vt"])
            assert packed.cpu().numpy().tobytes() == host_push
            B.handlePush(fmt, host_push)
            A.flush()
            B.flush()
            assert A.values().tobytes() == B.values().tobytes(), it
            assert A.values().tobytes() != init.tobytes()
            if case["ada"]:
                (aa, ad), (ba, bd) = A.adagrad_state(), B.adagrad_state()
                assert aa.tobytes() == ba.tobytes() and ad.tobytes() == bd.tobytes(), it
    finally:
        A.close()
        B.close()

"""A worker whose minibatch lists keys with repeats, entirely in HBM, against the reference-shaped
worker on the host.

The device worker holds occurrences (token ids with repeats, one gradient row per occurrence):
coalesce (keys only) -> handleFetchDevice of the unique keys -> unpack_fetch_device -> a gather
by the inverse -> a per-occurrence gradient -> coalesce -> pack_push_device -> pushDevice. The
host worker on a twin store does what the reference's does (Word2Vec.scala:246-300): a dict
accumulated per key in occurrence order from +0.0, the keys sorted, encode_matrix_push,
handlePush. The stores stay byte-equal, and the packed bytes are the host's push.
"""
import numpy as np
import pytest

import codec_cases as cc
import coalesce_expect as ce
from test_gpu_worker_iteration import KINDS, host_fetch, make_store

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def host_accumulate(keys, g):
    """The reference worker's HashMap: per key, the occurrences' rows added in list order from
    +0.0; returned with the keys sorted."""
    acc = {}
    zero = np.zeros(g.shape[1], g.dtype)
    with np.errstate(all="ignore"):
        for k, row in zip(keys.tolist(), g):
            acc[k] = acc.get(k, zero) + row
    ks = np.array(sorted(acc), np.int64)
    return ks, np.stack([acc[k] for k in ks.tolist()])


@pytest.mark.parametrize("case", KINDS, ids=lambda c: c["id"])
def test_worker_iteration_with_repeats(case):
    """The f32 (50 columns, int keys) and AdaGrad (200 columns, long keys) stores of
    tests/test_gpu_worker_iteration.py, 1 237 rows; 900 occurrences drawn from 301 rows; three
    iterations on one stream, one synchronise before each push."""
    from distml_amd import Coalescer, DeviceKeys, encode_matrix_push, pack_push_device, record_bytes, unpack_fetch_device
    rows, cols, first = case["rows"], case["cols"], case["first"]
    rng = np.random.default_rng(47)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    A, B = make_store(case, init), make_store(case, init)
    fmt = A.format
    push_rec, fetch_rec = record_bytes(fmt, cols)
    co = Coalescer(0)
    st = torch.cuda.Stream()
    n = 900
    try:
        for it in range(3):
            pool = first + rng.permutation(rows)[:301].astype(np.int64)
            keys = pool[rng.integers(0, 301, size=n)]
            hk = np.unique(keys)
            assert 200 < len(hk) <= 301
            dk = torch.from_numpy(keys.copy()).cuda()
            ukeys = torch.empty(n, dtype=torch.int64, device="cuda")
            ukeys2 = torch.empty(n, dtype=torch.int64, device="cuda")
            inv = torch.empty(n, dtype=torch.int32, device="cuda")
            fetched = torch.empty(n * fetch_rec // 4 + 1, dtype=torch.int32, device="cuda")[1:]  # 4 mod 16
            vals = torch.empty((n, cols), dtype=torch.float32, device="cuda")
            alpha = torch.empty((n, cols), dtype=torch.float32, device="cuda") if case["ada"] else None
            gsum = torch.empty(n * cols + 1, dtype=torch.float32, device="cuda")[1:]             # 4 mod 16
            packed = torch.empty(n * push_rec // 4 + 3, dtype=torch.int32, device="cuda")[3:]    # 12 mod 16
            step = torch.arange(n, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                m = co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), None, ukeys.data_ptr(), None, inv.data_ptr(), n,
                           stream=st.cuda_stream)  # the KeyList half: what to fetch
                assert m == len(hk)
                assert A.handleFetchDevice(fmt, DeviceKeys(ukeys.data_ptr(), m), fetched.data_ptr(), m * fetch_rec,
                                           stream=st.cuda_stream) == m * fetch_rec
                unpack_fetch_device(fmt, cols, fetched.data_ptr(), m, vals.data_ptr(),
                                    alpha.data_ptr() if case["ada"] else None, None, stream=st.cuda_stream)
                occ = vals[:m][inv.long()]  # every occurrence's row of the model
                grad = (occ * -0.125 + (step * 0.001 + (it + 1) * 0.0625)[:, None]).contiguous()
                assert co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), grad.data_ptr(), ukeys2.data_ptr(),
                              gsum.data_ptr(), None, m, stream=st.cuda_stream) == m
                assert pack_push_device(fmt, cols, DeviceKeys(ukeys2.data_ptr(), m), gsum.data_ptr(), m,
                                        packed.data_ptr(), m * push_rec, stream=st.cuda_stream) == m * push_rec
            st.synchronize()  # a push reads its buffers from the store's own streams
            A.pushDevice([packed.data_ptr()], [m * push_rec])
            # the host worker: a KeyList fetch, the per-occurrence gradient, the HashMap, one push
            fk, hv, ha = cc.unpack_expected(case, host_fetch(B, hk))
            assert ukeys[:m].cpu().numpy().tobytes() == ukeys2[:m].cpu().numpy().tobytes() == hk.tobytes() == fk.tobytes()
            assert (hk[inv.cpu().numpy()] == keys).all()
            assert vals[:m].cpu().numpy().tobytes() == hv.tobytes()
            if case["ada"]:
                assert alpha[:m].cpu().numpy().tobytes() == ha.tobytes()
            g = grad.cpu().numpy()
            sk, sv = host_accumulate(keys, g)
            assert sk.tobytes() == hk.tobytes()
            assert sv.tobytes() == ce.coalesce(keys, g)[2].tobytes()  # the HashMap is the model
            host_push = encode_matrix_push(sk, sv, case["kt"], case["vt"])
            assert packed[:m * push_rec // 4].cpu().numpy().tobytes() == host_push
            B.handlePush(fmt, host_push)
            A.flush()
            B.flush()
            assert A.values().tobytes() == B.values().tobytes(), it
            assert A.values().tobytes() != init.tobytes()
            if case["ada"]:
                (aa, ad), (ba, bd) = A.adagrad_state(), B.adagrad_state()
                assert aa.tobytes() == ba.tobytes() and ad.tobytes() == bd.tobytes(), it
    finally:
        co.close()
        A.close()
        B.close()


def test_coalesced_full_cover_is_an_identity_push(oracle):
    """Occurrences that cover every row of a plain f32 store, with repeats, in shuffled order:
    coalesced, they are one record per row in row order, which the store applies as an identity
    push (record r is row r, no key index). The shape is the 16 384 x 1 024 shard at which
    tests/test_gpu_parity.py asserts identity_pushes. After the flush dml_store_stats shows
    identity_pushes up by 1 and indexed_pushes by 0, and the shard equals the oracle fed the
    host worker's push."""
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, encode_matrix_push, pack_push_device
    rows, cols, extra = 16384, 1024, 3000
    fmt = DataDesc(1, 0, 1)
    rng = np.random.default_rng(61)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    keys = np.concatenate([np.arange(rows), rng.integers(0, rows, size=extra)]).astype(np.int64)
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    g = (rng.standard_normal((n, cols)) * 1e-3).astype(np.float32)
    s = DataStore(fmt, KeyRange(0, rows - 1), cols, async_push=True)
    co = Coalescer(0)
    try:
        s.load_values(init)
        dk, dg = torch.from_numpy(keys).cuda(), torch.from_numpy(g).cuda()
        ukeys = torch.empty(rows, dtype=torch.int64, device="cuda")
        gsum = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
        rec = 4 + 4 * cols
        packed = torch.empty(rows * rec, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), dg.data_ptr(), ukeys.data_ptr(), gsum.data_ptr(), None,
                      rows) == rows
        assert pack_push_device(fmt, cols, DeviceKeys(ukeys.data_ptr(), rows), gsum.data_ptr(), rows,
                                packed.data_ptr(), rows * rec) == rows * rec
        before = s.stats()
        s.pushDevice([packed.data_ptr()], [rows * rec])
        s.flush()
        after = s.stats()
        assert after["identity_pushes"] - before["identity_pushes"] == 1, (before, after)
        assert after["indexed_pushes"] - before["indexed_pushes"] == 0, (before, after)
        uk, _, sums = ce.coalesce(keys, g)
        assert uk.tobytes() == np.arange(rows, dtype=np.int64).tobytes()
        host_push = encode_matrix_push(uk, sums, 0, 1)
        assert packed.cpu().numpy().tobytes() == host_push
        o = oracle.OracleStore(1, 0, 1, 0, rows - 1, cols)
        o.data[:] = init
        assert o.push(host_push) == 0
        assert s.values().tobytes() == o.data.tobytes()
    finally:
        co.close()
        s.close()

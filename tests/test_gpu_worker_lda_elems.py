"""One LightLDA worker step (LightLDA.scala:224-239) wholly on the device and on one stream, with no
synchronize: the words' rows fetched into a plane, token moves computed from them, and the moves pushed
as element updates into the word-topic IntMatrixStore (300 x 1 000) and the topic-total IntArrayStore.
Three iterations, byte for byte against twin stores fed the host worker's pushes."""
import numpy as np
import pytest

from test_gpu_coalesce import _gpu  # noqa: F401  (the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def test_lda_worker_step_on_one_stream():
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, encode_array_push, encode_matrix_push
    W, T, n, first = 300, 1000, 900, 1000
    rng = np.random.default_rng(23)
    init = rng.integers(64, 200, size=(W, T)).astype(np.int32)
    fm, fa = DataDesc(1, 0, 0, False, True, False), DataDesc(0, 1, 0, False, True, False)
    wt, tot = ([DataStore(f, KeyRange(k0, k0 + r - 1), c) for _ in range(2)] for f, k0, r, c in ((fm, first, W, T), (fa, 0, T, 1)))
    co, st, keep = Coalescer(0), torch.cuda.Stream(), []
    try:
        for s in wt + tot:
            s.load_values(init if s in wt else init.sum(axis=0, dtype=np.int32).reshape(T, 1))
        for it in range(3):
            words = first + rng.integers(0, W, size=n).astype(np.int64)
            old = rng.integers(0, T, size=n).astype(np.int32)
            dk, do = torch.from_numpy(words).cuda(), torch.from_numpy(old).cuda()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                plane = torch.empty((n, T), dtype=torch.int32, device="cuda")
                wt[0].handleFetchPlanesDevice(fm, DeviceKeys(dk.data_ptr(), n), plane.data_ptr(), None, stream=st.cuda_stream)
                # the move: the token's new topic follows from the fetched count of its old one
                new = ((do + plane.gather(1, do.long()[:, None])[:, 0]) % T).int()
                cols = torch.stack([do, new], 1).contiguous()
                vals = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
                tk, tv = torch.cat([do, new]).long().contiguous(), vals.t().contiguous().view(-1)
                wt[0].handlePushElemsDevice(fm, co, DeviceKeys(dk.data_ptr(), n), cols.data_ptr(), vals.data_ptr(), 2, stream=st.cuda_stream)
                tot[0].handlePushElemsDevice(fa, co, DeviceKeys(tk.data_ptr(), 2 * n), None, tv.data_ptr(), 1, stream=st.cuda_stream)
            keep += [dk, do, plane, new, cols, vals, tk, tv]
            # the host worker: the same moves from the twin's rows, a dict of new - old rows, keys sorted
            nw = (old + wt[1].values()[words - first, old]) % T
            delta, tdelta = {}, {}
            for w, o, t in zip(words.tolist(), old.tolist(), nw.tolist()):
                row = delta.setdefault(w, np.zeros(T, np.int32))
                for topic, d in ((o, -1), (t, 1)):
                    row[topic] += d
                    tdelta[topic] = tdelta.get(topic, 0) + d
            ks, ts = sorted(delta), sorted(tdelta)
            wt[1].handlePush(fm, encode_matrix_push(np.array(ks, np.int64), np.stack([delta[k] for k in ks]), 0, 0))
            tot[1].handlePush(fa, encode_array_push(np.array(ts, np.int64), np.array([tdelta[t] for t in ts], np.int32), 1, 0))
        for a, b in (wt, tot):
            a.flush(), b.flush()
            assert a.values().tobytes() == b.values().tobytes()
        assert wt[0].values().tobytes() != init.tobytes()
    finally:
        co.close()
        [s.close() for s in wt + tot]

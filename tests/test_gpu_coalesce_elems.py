"""dml_coalesce_elems_device (Coalescer.run_elems), byte for byte against numpy: np.add.at on an
int64 plane reduced mod 2^32, keys from np.unique, records from encode_matrix_push. Every output
is a geom.OutArena between poison at 4 or 12 mod 16 (the 8-byte-aligned key plane at 8), every
input a geom.Arena compared unchanged afterwards."""
import ctypes as C

import numpy as np
import pytest

import geom
from test_gpu_coalesce import _gpu, co, same  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from distml_amd import DataDesc, DeviceKeys, _lib, encode_matrix_push  # noqa: E402

SLICE, NEVER = _lib.DML_COALESCE_ELEMS_SLICE, 2 ** 31
POOL = np.concatenate([np.arange(-150, 0), (1 << 32) + np.arange(150)]).astype(np.int64)


def fmt(kt):
    return DataDesc(1, kt, 0, False, True, False)


def moves(n, cols, per, seed):
    """n occurrences of `per` elements; columns drawn from [-1, cols], so both ends fall outside
    the row; deltas up to 2^30, so sums wrap. n < 100: one key, a segment of n. Else segments of
    1 500, 65 (every element on one column, each 2^30: all lanes collide and the sum wraps), 64,
    two lone keys whose elements are all -1 / all `cols`, and repeats over POOL, shuffled."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-1, cols + 1, size=(n, per)).astype(np.int32)
    v = rng.integers(-2 ** 30, 2 ** 30, size=(n, per)).astype(np.int32)
    if n < 100:
        return np.full(n, POOL[seed % len(POOL)]), c, v
    keys = np.concatenate([np.full(1500, -1000), np.full(65, (1 << 33) + 1), np.full(64, -7000), [(1 << 32) + 999, 5000],
                           POOL[rng.integers(0, len(POOL), size=n - 1631)]]).astype(np.int64)
    c[1500:1565], v[1500:1565] = cols // 2, 2 ** 30
    c[1629], c[1630] = -1, cols
    p = rng.permutation(n)
    return keys[p], c[p], v[p]


def expect(keys, c, v, cols, kt, records):
    """(distinct keys, inverse, output bytes, (segments of >= 2, their occurrences))."""
    uk, inv = np.unique(keys, return_inverse=True)
    plane = np.zeros((len(uk), cols), np.int64)
    ok = (c >= 0) & (c < cols)
    np.add.at(plane, (np.broadcast_to(inv[:, None], c.shape)[ok], c[ok]), v[ok].astype(np.int64))
    rows = (plane & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    cnt = np.bincount(inv)
    out = encode_matrix_push(uk, rows, kt, 0) if records else rows.tobytes()
    return uk, inv.astype(np.int32), out, (int((cnt >= 2).sum()), int(cnt[cnt >= 2].sum()))


def upload(keys, c, v, lead):
    return geom.pack([keys.tobytes()], lead & 8), geom.pack([c.tobytes()], lead), geom.pack([v.tobytes()], 16 - lead)


def outputs(m, n, nbytes, lead):
    return geom.OutArena(nbytes, lead).upload(), geom.OutArena(m * 8, 8).upload(), geom.OutArena(n * 4, 16 - lead).upload()


@pytest.mark.parametrize("records", [False, True], ids=["rows", "records"])
@pytest.mark.parametrize("per", [1, 2, 16])
@pytest.mark.parametrize("cols", [1, 3, 250, 1000, SLICE, SLICE + 1, 2 * SLICE + 3])
def test_parity(co, cols, per, records):
    """Both routes (long_min never, then 2) for n = 1, 63, 64, 65 and 3 000; the key width
    alternates with n and the case, so either width meets every n, cols and per_occ."""
    for i, n in enumerate([1, 63, 64, 65, 3000]):
        kt, lead = (i + per + records) % 2, (4, 12)[i % 2]
        keys, c, v = moves(n, cols, per, seed=cols + per + i)
        uk, inv, want, longs = expect(keys, c, v, cols, kt, records)
        ka, ca, va = upload(keys, c, v, lead)
        for thr, route in ((NEVER, (0, 0)), (2, longs)):
            co.set_long_min(thr)
            oo, ko, io = outputs(len(uk), n, len(want), lead)
            got = co.run_elems(fmt(kt), cols, DeviceKeys(ka.ptrs[0], n), ca.ptrs[0], va.ptrs[0], per, oo.ptr, len(want),
                               records, ko.ptr, io.ptr)
            what = (n, kt, thr)
            assert got == (len(uk), len(want)), what
            assert co.route() == route, what
            for a, b in ((oo, want), (ko, uk.tobytes()), (io, inv.tobytes())):
                same(a.read(), b, what)
                a.untouched([(0, len(b))])
        for a in (ka, ca, va):
            a.check()
    co.set_long_min(0)


@pytest.mark.parametrize("records", [False, True], ids=["rows", "records"])
def test_capacity(co, records):
    """cap_bytes one byte short: DML_E_CAPACITY, m and the needed bytes reported, and no byte
    of the output, the keys or the inverse has changed."""
    n, cols, per, kt = 3000, 250, 2, 1
    keys, c, v = moves(n, cols, per, seed=5)
    uk, _, want, _ = expect(keys, c, v, cols, kt, records)
    ka, ca, va = upload(keys, c, v, 4)
    oo, ko, io = outputs(len(uk), n, len(want), 12)
    m, ln = C.c_int64(-7), C.c_int64(-7)
    rc = _lib.load().dml_coalesce_elems_device(co._h, C.byref(fmt(kt).to_c()), cols, 0, ka.ptrs[0], n, per, ca.ptrs[0],
                                               va.ptrs[0], int(records), oo.ptr, len(want) - 1, ko.ptr, io.ptr,
                                               C.byref(m), C.byref(ln), None)
    assert (rc, m.value, ln.value) == (_lib.DML_E_CAPACITY, len(uk), len(want))
    for a in (oo, ko, io):
        a.read()
        a.untouched([])


def test_lda_worker_step():
    """A LightLDA worker (LightLDA.scala:224-239) on 300 words x 1 000 topics, 900 tokens, int
    keys: the moves through run_elems(records=True) and pushDevice, against a twin store fed the
    host worker's push (a dict of new - old rows, keys sorted, encode_matrix_push, handlePush)."""
    from distml_amd import Coalescer, DataStore, KeyRange
    W, T, n, first = 300, 1000, 900, 1000
    rng = np.random.default_rng(17)
    init = rng.integers(64, 200, size=(W, T)).astype(np.int32)
    f = fmt(0)
    A, B, co = DataStore(f, KeyRange(first, first + W - 1), T), DataStore(f, KeyRange(first, first + W - 1), T), Coalescer(0)
    try:
        A.load_values(init)
        B.load_values(init)
        for it in range(3):
            words = first + rng.integers(0, W, size=n).astype(np.int64)
            topics = rng.integers(0, T, size=(n, 2)).astype(np.int32)  # (old, new)
            dk, dc = torch.from_numpy(words).cuda(), torch.from_numpy(topics).cuda()
            dv = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
            packed = torch.empty(n * (4 + 4 * T) // 4 + 3, dtype=torch.int32, device="cuda")[3:]  # 12 mod 16
            torch.cuda.synchronize()
            m, nbytes = co.run_elems(f, T, DeviceKeys(dk.data_ptr(), n), dc.data_ptr(), dv.data_ptr(), 2,
                                     packed.data_ptr(), packed.numel() * 4, records=True)
            A.pushDevice([packed.data_ptr()], [nbytes])
            delta = {}
            for w, (old, new) in zip(words.tolist(), topics.tolist()):
                row = delta.setdefault(w, np.zeros(T, np.int32))
                row[old] -= 1
                row[new] += 1
            ks = sorted(delta)
            host_push = encode_matrix_push(np.array(ks, np.int64), np.stack([delta[k] for k in ks]), 0, 0)
            assert m == len(ks) and packed[:nbytes // 4].cpu().numpy().tobytes() == host_push
            B.handlePush(f, host_push)
            A.flush()
            B.flush()
            assert A.values().tobytes() == B.values().tobytes(), it
        assert A.values().tobytes() != init.tobytes()
    finally:
        co.close()
        A.close()
        B.close()

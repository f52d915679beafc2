"""GPU, one process: the two kernels of dml_group_pull through dml_diag_pull_kernels — the key
partition (k_pull_count / _scan / _scatter) and the request-order permutation
(k_pull_unsplit) — against numpy: a stable partition by owner and a record permutation.

Outputs of the permutation sit in a geom.OutArena (poisoned guard bands, checked byte for
byte), inputs in a geom.Arena, both at the four offsets from a 16-byte boundary."""
import ctypes as C

import numpy as np
import pytest

import fetch_cases as fc
import geom

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7
TILE = 1024  # keys per block of the partition kernels (kPullTile)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def step_of(total, world):
    from distml_amd.datadesc import KeyRange
    return KeyRange(0, total - 1).linearSplit(world)[0].size()


def np_partition(keys, total, world):
    """(keys by owner in list order, slot per list index, kept index per list index, counts
    with the dropped count last)."""
    keys = np.asarray(keys, np.int64)
    inside = (keys >= 0) & (keys < total)
    owner = np.where(inside, keys // step_of(total, world), world)
    order = np.argsort(owner, kind="stable")
    nkept = int(inside.sum())
    slot = np.full(len(keys), -1, np.int64)
    slot[order[:nkept]] = np.arange(nkept)
    kept = np.where(inside, np.arange(len(keys)) - np.cumsum(~inside), -1)
    return keys[order[:nkept]], slot, kept, np.bincount(owner, minlength=world + 1)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() if len(a) else torch.zeros(1, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    return t


def run_diag(keys, total, world, src_ptr=0, dst_ptr=0, rec_bytes=0, variant=0):
    from distml_amd import _lib
    L = _lib.load()
    n = len(keys)
    dk = dev(np.asarray(keys, np.int64))
    part, slot, kept = (torch.full((max(n, 1),), SENTINEL, dtype=torch.int64, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    counts = (C.c_int64 * (world + 1))()
    ms = (C.c_float(), C.c_float())
    rc = L.dml_diag_pull_kernels(C.c_void_p(dk.data_ptr()), n, total, world, C.c_void_p(part.data_ptr()),
                                 C.c_void_p(slot.data_ptr()), C.c_void_p(kept.data_ptr()), counts,
                                 C.c_void_p(src_ptr or None), C.c_void_p(dst_ptr or None), rec_bytes, variant, None,
                                 C.byref(ms[0]), C.byref(ms[1]))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return part.cpu().numpy()[:n], slot.cpu().numpy()[:n], kept.cpu().numpy()[:n], np.array(list(counts))


def key_patterns(n, total, world, rng):
    step = step_of(total, world)
    last = world - 1
    lo, hi = last * step, total - 1
    out = {"one_owner": rng.integers(lo, hi + 1, size=n),
           "dropped": np.resize(np.array([-1, total, 1 << 40, -(1 << 33), (1 << 32) + 1, total + 5]), n),
           "alternating": (np.arange(n) % world) * step + (np.arange(n) // world) % (total - last * step),
           "mixed": np.where(rng.random(n) < 0.2, rng.choice(np.array([-1, total, 1 << 40, -5]), size=n),
                             rng.integers(0, total, size=n))}
    return {k: v.astype(np.int64) for k, v in out.items()}


@pytest.mark.parametrize("world", [1, 3, 64])
def test_partition(world):
    """Stable partition, slots, kept indices and counts at 0, 1, 255, 256, 257 keys, one key
    either side of one and of several block tiles, and many blocks; keys all to one owner, all
    dropped (negative, total_rows, past 2^32 and 2^40), alternating owners, and mixed."""
    total = 1024  # world 64: shards of 16 rows
    rng = np.random.default_rng(world)
    for n in (0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE + 1, 300 * TILE + 77):
        for name, keys in key_patterns(n, total, world, rng).items():
            want = np_partition(keys, total, world)
            got = run_diag(keys, total, world)
            nk = len(want[0])
            what = (world, n, name)
            assert got[3].tolist() == want[3].tolist(), what
            assert np.array_equal(got[0][:nk], want[0]) and (got[0][nk:] == SENTINEL).all(), what
            assert np.array_equal(got[1], want[1]), what
            assert np.array_equal(got[2], want[2]), what


def edge_counts(rec_bytes):
    from distml_amd import _lib
    out = []
    for unit in (_lib.DML_PULL_WAVE_BYTES, _lib.DML_PULL_BLOCK_BYTES):
        n = int(np.lcm(rec_bytes, unit)) // rec_bytes  # records until a record end meets a tile end
        out += [n - 1, n, n + 1]
    return out


@pytest.mark.parametrize("recdw", [3, 4, 5, 68, 201, 257, 401, 769, 1025])
def test_unsplit(recdw):
    """Record j of the output is the record of the j-th kept key, for records of 3 .. 1025
    dwords; 0, 1, 255, 256, 257 kept records and one record either side of the kernel's wave
    and block tiles; input and output at 0 / 4 / 8 / 12 bytes past a 16-byte boundary; values
    with -0.0, denormals, Inf and NaN payloads; all three load variants; guard bands intact."""
    from distml_amd import _lib
    assert (_lib.DML_PULL_WAVE_BYTES, _lib.DML_PULL_BLOCK_BYTES) == (1024, 4096)
    total, world, rec = 5000, 3, 4 * recdw
    rng = np.random.default_rng(recdw)
    counts = sorted(set([0, 1, 255, 256, 257] + edge_counts(rec)))
    sp = np.concatenate([fc.specials(1), fc.specials(3).view("<u4"), fc.specials(0)])
    for ci, nk in enumerate(counts):
        # nk kept keys in a seeded order, a dropped key after every seventh
        keys = rng.integers(0, total, size=nk).astype(np.int64)
        keys = np.insert(keys, np.arange(7, nk, 7), -1)
        _, slot, kept, _ = np_partition(keys, total, world)
        perm = np.empty(nk, np.int64)
        perm[kept[kept >= 0]] = slot[kept >= 0]
        src = rng.integers(0, 1 << 32, size=(nk, recdw), dtype=np.uint64).astype("<u4")
        if nk:
            src.reshape(-1)[rng.integers(0, src.size, size=min(src.size, 64))] = np.resize(sp, min(src.size, 64))
        want = src[perm].tobytes()
        leads = [(lead, geom.LEADS[(i + 1 + ci) % 4]) for i, lead in enumerate(geom.LEADS)]
        for variant, (lead_out, lead_in) in [(0, p) for p in leads] + [(1, leads[1]), (2, leads[2])]:
            arena = geom.pack([src.tobytes()], lead_in)
            out = geom.OutArena(len(want), lead_out).upload()
            run_diag(keys, total, world, arena.ptrs[0], out.ptr, rec, variant)
            got = out.read()
            what = (recdw, nk, variant, lead_out, lead_in)
            if got.tobytes() != want:
                bad = np.flatnonzero(got != np.frombuffer(want, np.uint8))
                raise AssertionError((what, "first differing byte", int(bad[0]), "of", len(want), "count", bad.size))
            out.untouched([(0, len(want))])
            arena.check()


def test_bad_arguments():
    from distml_amd import _lib
    L = _lib.load()
    counts = (C.c_int64 * 66)()
    k = dev(np.arange(4, dtype=np.int64))
    for args in ((k.data_ptr(), -1, 10, 2), (k.data_ptr(), 4, 0, 2), (k.data_ptr(), 4, 10, 65), (k.data_ptr() + 4, 4, 10, 2)):
        rc = L.dml_diag_pull_kernels(C.c_void_p(args[0]), args[1], args[2], args[3], C.c_void_p(k.data_ptr()), None, None,
                                     counts, None, None, 0, 0, None, None, None)
        assert rc == _lib.DML_E_INVALID_ARG, args

"""dml_records_expand_device (expand_fetch_device): the planes are cc.unpack_expected(records)[...][inverse]
of host-made records (random words, NaN payloads, -0.0), byte for byte; arenas between canaries."""
import ctypes as C

import numpy as np
import pytest

import codec_cases as cc
import fetch_cases as fc
import geom
from test_gpu_coalesce import _gpu, desc, same  # noqa: F401  (_gpu: the module's GPU gate)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ADA = fc._case("ada", 1, 1, 1, 200, 0, 0, True)
CASES = [(fc._case("f32", 1, 0, 1, 50, 0, 0), "v"), (ADA, "va"), (ADA, "v"), (ADA, "a"),
         (fc._case("f64", 1, 0, 3, 129, 0, 0), "v"), (fc._case("i32", 1, 1, 0, 1000, 0, 0), "v"),
         (fc._case("af32", 0, 1, 1, 1, 0, 0), "v"), (fc._case("af32ref", 0, 0, 1, 1, 0, 0, False, True), "v"),
         (fc._case("af64", 0, 0, 3, 1, 0, 0), "v"), (fc._case("ai32", 0, 1, 0, 1, 0, 0), "v")]


def records(case, m, seed=0):
    """m fetch records of random words; the planes they hold."""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, size=m * fc.record_bytes(case) // 4, dtype=np.uint64).astype("<u4")
    words[rng.choice(words.size, size=min(words.size, 24), replace=False)] = np.resize(fc.specials(1), min(words.size, 24))
    _, vals, alpha = cc.unpack_expected(case, words.tobytes())
    return words.tobytes(), {"v": vals, "a": alpha}


def run(case, planes, rec, want, m, inv, lead, stream=None, what=()):
    """One expand into canary arenas. Rows whose inverse is outside [0, m) must stay canary."""
    from distml_amd import expand_fetch_device
    n, ok = len(inv), (inv >= 0) & (inv < m)
    ra, ia = geom.pack([rec], 16 - lead), geom.pack([inv.tobytes()], lead)
    outs = {p: geom.OutArena(n * want[p][0].nbytes, (lead + 8 * i) % 16).upload() for i, p in enumerate(planes)}
    expand_fetch_device(desc(case["dt"], case["kt"], case["vt"], case["ada"]), case["cols"], ra.ptrs[0], m, ia.ptrs[0], n,
                        outs["v"].ptr if "v" in outs else None, outs["a"].ptr if "a" in outs else None, stream=stream,
                        flags=cc.flags(case))
    torch.cuda.synchronize()
    for p, o in outs.items():
        rowb = want[p][0].nbytes
        same(o.read().reshape(n, rowb)[ok].reshape(-1), want[p][inv[ok]].tobytes(), (p,) + tuple(what))
        o.untouched([(j * rowb, (j + 1) * rowb) for j in np.flatnonzero(ok)])
    ra.check()
    ia.check()


@pytest.mark.parametrize("case,planes", CASES, ids=[c["store"] + "-" + p for c, p in CASES])
def test_layouts(case, planes):
    """Planes that end one row around three wave runs and one block; a random inverse with 0 and m - 1; then
    -1, m and INT32_MIN among the valid entries: those rows stay canary, every other row is right."""
    from distml_amd import _lib
    m, rng = 37, np.random.default_rng(11)
    rec, want = records(case, m, seed=len(planes))
    ns = cc.edge_counts(want[planes[0]][0].nbytes, _lib.DML_CODEC_WAVE_BYTES, _lib.DML_CODEC_BLOCK_BYTES)
    for i, n in enumerate(ns):
        inv = rng.integers(0, m, size=n).astype(np.int32)
        inv[[0, n - 1]] = (m - 1, 0) if n > 1 else 0
        run(case, planes, rec, want, m, inv, (4, 12)[i % 2], torch.cuda.Stream().cuda_stream if i % 2 else None, what=(n,))
    inv[[0, 7, 8, 20, n - 1]] = [-1, m, -(1 << 31), m + 1000, -1]
    run(case, planes, rec, want, m, inv, 12, what=("bad inverse",))


def test_refusals():
    """Each argument error (argument index, value), the first also on a stream; nothing written; then it works."""
    from distml_amd import _lib
    m, n, cols = 5, 9, ADA["cols"]
    rec, want = records(ADA, m)
    inv = (np.arange(n) % m).astype(np.int32)
    ra, ia = geom.pack([rec], 4), geom.pack([inv.tobytes()], 12)
    vo, ao = geom.OutArena(n * cols * 4, 4).upload(), geom.OutArena(n * cols * 4, 12).upload()
    good = [desc(1, 1, 1, True), cols, 0, ra.ptrs[0], m, ia.ptrs[0], n, vo.ptr, ao.ptr]
    # m < 0, n < 0, null inverse, misaligned values, values over the records, an alpha plane without AdaGrad
    cases = [(4, -1), (6, -1), (5, 0), (7, vo.ptr + 1), (7, ra.ptrs[0] + 4), (0, desc(1, 1, 1))]
    for stream in (None, torch.cuda.Stream().cuda_stream):
        for at, value in cases if stream is None else cases[:1]:
            a = good[:at] + [value] + good[at + 1:]
            assert _lib.load().dml_records_expand_device(C.byref(a[0].to_c()), *a[1:], stream) == _lib.DML_E_INVALID_ARG, at
    for a in (vo, ao):
        a.read()
        a.untouched([])
    run(ADA, "va", rec, want, m, inv, 4, what=("after the refusals",))

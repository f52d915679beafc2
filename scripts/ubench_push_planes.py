#!/usr/bin/env python3
"""Timing of the plane push (dml_store_push_planes_device) against, in the same
process, (a) the chain it replaces for a worker on the store's GPU: Coalescer.run_packed into push
records, the worker's stream synchronisation, pushDevice of the records and the flush, without
(`chain`) and with (`chain_range`) a declared key range; and (b) the box's plain copy of n + 2 m
row-sizes of bytes (dml_diag_stream, copy = 1), the bytes a direct route has to move.

The plane push's shard kernels run on the store's apply stream, not on the caller's, so both routes
are timed the same way: a HIP event on the caller's stream in front, the calls as a worker makes
them, the store's flush, and an event behind (the host waits inside count: the coalescer's wait for
the distinct count in both, the worker's synchronize in the chain). `planes_range` is the plane push
with the key range declared. Per shape every candidate is warmed up, the two routes' final shard
bytes (AdaGrad: alpha and delta too) are compared on twin stores, then --rounds rounds alternate
the candidates; a round's figure is the median of --calls calls. One JSON line per shape goes to
--out (default profiles/push_planes_ubench.jsonl).

Shapes: 200 f32 columns at n = 2^20 occurrences, (x4) four per key, (distinct) every key once,
(zipf) a Zipf(1.1) list; the same three on an AdaGrad store (ada-x4, ...); (arr) a cols = 1 float
array at n = 2^24.

  python scripts/ubench_push_planes.py [--shapes x4,distinct,zipf,ada-x4,ada-distinct,ada-zipf,arr]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ubench_coalesce import emit, make_keys, rounds_of, timed  # noqa: E402

SHAPES = ("x4", "distinct", "zipf", "ada-x4", "ada-distinct", "ada-zipf", "arr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_planes_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, _lib, record_bytes
    assert torch.cuda.is_available(), "ubench_push_planes needs the GPU"
    L = _lib.load()
    for name in args.shapes.split(","):
        ada = name.startswith("ada-")
        keys, cols = make_keys(name.replace("ada-", ""), np.random.default_rng(5), np)
        n, m, rows = len(keys), len(np.unique(keys)), int(keys.max()) + 1
        fmt = DataDesc(1 if cols > 1 else 0, 1, 1, False, True, ada)
        R, row = record_bytes(fmt, cols)[0], 4 * cols

        def store():
            s = DataStore(fmt, KeyRange(0, rows - 1), cols)
            s.rand(3)
            ada and s.setAlpha(0.025, 0.0001, 1.5)
            return s

        a, b = store(), store()  # the chain's and the plane push's
        dk = torch.from_numpy(keys).cuda()
        vals = torch.randn((n, cols), dtype=torch.float32, device="cuda") * 0.01
        recs = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        moved = (n + 2 * m) * row
        src = torch.empty(moved, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty(moved, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        co, cor = Coalescer(0), Coalescer(0)
        cor.set_key_range(0, rows)
        torch.cuda.synchronize()

        def chain(c):
            def go():
                assert c.run_packed(fmt, cols, DeviceKeys(dk.data_ptr(), n), vals.data_ptr(), recs.data_ptr(), m * R,
                                    stream=st.cuda_stream) == (m, m * R)
                st.synchronize()  # a push reads its buffers from the store's own streams
                a.pushDevice([recs.data_ptr()], [m * R])
                a.flush()
            return timed(st, go)

        def planes(c):
            def go():
                b.handlePushPlanesDevice(fmt, c, DeviceKeys(dk.data_ptr(), n), vals.data_ptr(), stream=st.cuda_stream)
                b.flush()
            return timed(st, go)

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), moved, C.c_void_p(st.cuda_stream), C.byref(ms)) == 0
            return ms.value

        chain(co), planes(co), chain(cor), planes(cor)  # two calls each: the same bytes on both stores
        assert a.values().tobytes() == b.values().tobytes(), name
        assert not ada or all(x.tobytes() == y.tobytes() for x, y in zip(a.adagrad_state(), b.adagrad_state())), name
        assert not ada or a.maxDelta() == b.maxDelta(), name
        cands = dict(planes=lambda: planes(co), planes_range=lambda: planes(cor), chain=lambda: chain(co),
                     chain_range=lambda: chain(cor), copy=copy)
        per = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per.items()}
        emit(dict(shape=name, n=n, m=m, rows=rows, cols=cols, ada=ada, row_bytes=row, direct_bytes=moved,
                  copy_gbs=round(2 * moved / best["copy"] / 1e6, 1),
                  planes_over_copy=round(best["planes"] / best["copy"], 3),
                  chain_over_planes=round(best["chain"] / best["planes"], 3),
                  chain_range_over_planes_range=round(best["chain_range"] / best["planes_range"], 3)), per, args.out)
        for x in (co, cor, a, b):
            x.close()
        del dk, vals, recs, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

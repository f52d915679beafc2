#!/usr/bin/env python3
"""Timing of the plane fetch (dml_store_fetch_planes_device) against, in the same
process, (a) the three-call chain it replaces for a worker on the store's GPU: keys-only
Coalescer.run, dml_store_fetch_device of the distinct keys and dml_records_expand_device, without
(`chain`) and with (`chain_range`) a declared key range; and (b) the box's plain copy of the
planes' bytes (dml_diag_stream, copy = 1: it reads and writes them once, as the fetch does).

`planes` is the shipped launch; `planes_d1`, `planes_d2`, `planes_d4` are the depths of
DML_KNOB_FETCH_PLANES. Everything is timed by HIP events on the caller's stream, around the calls
as a worker makes them (the chain's figure includes the host's wait for the distinct count).
Per shape every candidate is warmed up, the new planes are compared with the chain's, then
--rounds rounds alternate the candidates; a round's figure is the median of --calls calls.
One JSON line per shape goes to --out (default profiles/fetch_planes_ubench.jsonl).

Shapes: 200 f32 columns at n = 2^20 occurrences, (x4) four per key, (distinct) every key once,
(zipf) a Zipf(1.1) list; the same three on an AdaGrad store, both planes (ada-x4, ...); (i32)
1 000 int32 columns at 65 536 occurrences of 262 144 rows; (arr) a cols = 1 float array at n = 2^24.

  python scripts/ubench_fetch_planes.py [--shapes x4,distinct,zipf,ada-x4,ada-distinct,ada-zipf,i32,arr]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ubench_coalesce import emit, make_keys, rounds_of, timed  # noqa: E402

SHAPES = ("x4", "distinct", "zipf", "ada-x4", "ada-distinct", "ada-zipf", "i32", "arr")
KNOB = 4  # DML_KNOB_FETCH_PLANES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_planes_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import (Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, _lib, expand_fetch_device,
                            record_bytes)
    assert torch.cuda.is_available(), "ubench_fetch_planes needs the GPU"
    L = _lib.load()
    for name in args.shapes.split(","):
        ada = name.startswith("ada-")
        rng = np.random.default_rng(5)
        if name == "i32":
            keys, cols, vt = rng.integers(0, 262144, size=65536).astype(np.int64), 1000, 0
        else:
            keys, cols = make_keys(name.replace("ada-", ""), rng, np)
            vt = 1
        n, m, rows = len(keys), len(np.unique(keys)), int(keys.max()) + 1
        fmt = DataDesc(1 if cols > 1 else 0, 1, vt, False, True, ada)
        s = DataStore(fmt, KeyRange(0, rows - 1), cols)
        s.rand(3)
        if ada:
            s.setAlpha(0.025, 0.0001, 1.5)
        F, planes, row = record_bytes(fmt, cols)[1], 2 if ada else 1, 4 * cols
        dk = torch.from_numpy(keys).cuda()
        ukeys = torch.empty(n, dtype=torch.int64, device="cuda")
        inv = torch.empty(n, dtype=torch.int32, device="cuda")
        fetched = torch.empty(m * F // 4, dtype=torch.int32, device="cuda")
        occ = [torch.empty((n, cols), dtype=torch.int32, device="cuda") for _ in range(planes)]
        new = [torch.empty((n, cols), dtype=torch.int32, device="cuda") for _ in range(planes)]
        moved = planes * n * row
        src = torch.empty(moved, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty(moved, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        co, cor = Coalescer(0), Coalescer(0)
        cor.set_key_range(0, rows)
        torch.cuda.synchronize()

        def chain(c):
            def go():
                assert c.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), None, ukeys.data_ptr(), None, inv.data_ptr(), n,
                             stream=st.cuda_stream) == m
                s.handleFetchDevice(fmt, DeviceKeys(ukeys.data_ptr(), m), fetched.data_ptr(), m * F, stream=st.cuda_stream)
                expand_fetch_device(fmt, cols, fetched.data_ptr(), m, inv.data_ptr(), n, occ[0].data_ptr(),
                                    occ[1].data_ptr() if ada else None, stream=st.cuda_stream)
            return timed(st, go)

        def fetch_planes(depth):
            s.set_knob(KNOB, depth)
            return timed(st, lambda: s.handleFetchPlanesDevice(fmt, DeviceKeys(dk.data_ptr(), n), new[0].data_ptr(),
                                                                new[1].data_ptr() if ada else None, stream=st.cuda_stream))

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), moved, C.c_void_p(st.cuda_stream), C.byref(ms)) == 0
            return ms.value

        chain(co)
        for depth in (1, 2, 4, 0):
            for p in new:
                p.fill_(-1)
            torch.cuda.synchronize()
            fetch_planes(depth)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(new, occ)), (name, depth)  # the chain's planes, bit for bit
        cands = dict(planes=lambda: fetch_planes(0), planes_d1=lambda: fetch_planes(1), planes_d2=lambda: fetch_planes(2),
                     planes_d4=lambda: fetch_planes(4), chain=lambda: chain(co), chain_range=lambda: chain(cor), copy=copy)
        per = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per.items()}
        emit(dict(shape=name, n=n, m=m, rows=rows, cols=cols, ada=ada, value_type=vt, row_bytes=row, plane_bytes=moved,
                  planes_gbs=round(2 * moved / best["planes"] / 1e6, 1), copy_gbs=round(2 * moved / best["copy"] / 1e6, 1),
                  planes_over_copy=round(best["planes"] / best["copy"], 3),
                  chain_over_planes=round(best["chain"] / best["planes"], 3),
                  chain_range_over_planes=round(best["chain_range"] / best["planes"], 3)), per, args.out)
        for x in (co, cor, s):
            x.close()
        del dk, ukeys, inv, fetched, occ, new, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

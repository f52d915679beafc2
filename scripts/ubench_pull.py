#!/usr/bin/env python3
"""Timing of the collective group pull's own kernels on one GPU, through
dml_diag_pull_kernels: the key partition (k_pull_count / _scan / _scatter) over random keys
at world 8, and the request-order permutation k_pull_unsplit in its load variants (by record
length, dword gathers, 16-byte loads) against the box's plain copy (dml_diag_stream, copy = 1)
of the same bytes; then the world-1 dml_group_pull call against dml_store_fetch_device on the
same keys (both synchronous, wall time).

Per shape every variant is warmed up, then three rounds alternate the variants in one
process; a round's figure is the median of --calls runs. One JSON line per shape and variant
goes to --out (default profiles/pull_group.jsonl); rates count the bytes once read and once
written. The exchanges' xGMI time is not measured here: one GPU has no peer.

  python scripts/ubench_pull.py [--shapes part1m,part32m,cfg4,w256,cfg4ada,cfg5,array,world1] [--calls 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORLD = 8
PARTITION = {"part1m": 1_000_000, "part32m": 32_000_000}
# name: (record dwords, records, model rows)
UNSPLIT = {"cfg4": (201, 1_250_000, 1_250_000), "cfg4ada": (401, 1_250_000, 1_250_000),
           "cfg5": (1001, 65_536, 1_000_000), "array": (3, 1_000_000, 1_000_000_000),
           # between config 4's record and its AdaGrad record, for the load-path threshold
           "w256": (257, 1_000_000, 1_000_000)}
VARIANTS = [("k_pull_unsplit", 0), ("k_pull_unsplit/dword-gather", 1), ("k_pull_unsplit/16-byte-loads", 2)]
DEFAULT = "part1m,part32m,cfg4,w256,cfg4ada,cfg5,array,world1"


def rounds(runs, nrounds, calls):
    for _, f in runs:
        for _ in range(3):
            f()
    per = {v: [] for v, _ in runs}
    for _ in range(nrounds):
        for v, f in runs:
            per[v].append(statistics.median(f() for _ in range(calls)))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pull_group.jsonl"))
    args = ap.parse_args()
    import torch
    from distml_amd import DataDesc, _lib
    assert torch.cuda.is_available(), "ubench_pull needs the GPU"
    L = _lib.load()
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def diag(keys, total, part, src=None, dst=None, rec=0, variant=0):
        counts = (C.c_int64 * (WORLD + 1))()
        mp, mu = C.c_float(), C.c_float()
        rc = L.dml_diag_pull_kernels(C.c_void_p(keys.data_ptr()), keys.numel(), total, WORLD, C.c_void_p(part.data_ptr()),
                                     None, None, counts, C.c_void_p(src.data_ptr() if src is not None else None),
                                     C.c_void_p(dst.data_ptr() if dst is not None else None), rec, variant, None,
                                     C.byref(mp), C.byref(mu))
        assert rc == 0, _lib.last_error()
        return mp.value, mu.value

    def copy_ms(dst, src, nbytes):
        ms = C.c_float()
        assert L.dml_diag_stream(1, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes & ~15, None,
                                 C.byref(ms)) == 0
        return ms.value

    for name in args.shapes.split(","):
        g = torch.Generator(device="cuda").manual_seed(11)
        if name in PARTITION:
            n, total = PARTITION[name], 1_000_000_000
            keys = torch.randint(0, total, (n,), dtype=torch.int64, device="cuda", generator=g)
            part = torch.empty(n, dtype=torch.int64, device="cuda")
            ref = torch.empty(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            per = rounds([("partition", lambda: diag(keys, total, part)[0]),
                          ("copy", lambda: copy_ms(ref, keys, 8 * n))], args.rounds, args.calls)
            ceil = min(per["copy"])
            for v in per:
                best = min(per[v])
                emit(shape=name, keys=n, world=WORLD, variant=v, round_ms=[round(x, 4) for x in per[v]],
                     best_ms=round(best, 4), mkeys_per_s=round(n / best / 1e3, 1), of_copy=round(ceil / best, 3))
            del keys, part, ref
        elif name in UNSPLIT:
            recdw, n, total = UNSPLIT[name]
            nbytes = 4 * recdw * n
            keys = torch.randint(0, total, (n,), dtype=torch.int64, device="cuda", generator=g)
            part = torch.empty(n, dtype=torch.int64, device="cuda")
            src = torch.randint(0, 1 << 31, (nbytes // 4 + 4,), dtype=torch.int32, device="cuda", generator=g)
            dst = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
            ref = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            outs = []
            for _, k in VARIANTS:  # the same bytes from every variant
                dst.zero_()
                torch.cuda.synchronize()
                diag(keys, total, part, src, dst, 4 * recdw, k)
                outs.append(dst.clone())
            assert all(torch.equal(o, outs[0]) for o in outs), name
            del outs
            runs = [(v, (lambda k=k: diag(keys, total, part, src, dst, 4 * recdw, k)[1])) for v, k in VARIANTS]
            runs.append(("copy", lambda: copy_ms(ref, src, nbytes)))
            per = rounds(runs, args.rounds, args.calls)
            ceil = min(per["copy"])
            for v in per:
                best = min(per[v])
                emit(shape=name, record_dwords=recdw, records=n, variant=v, out_bytes=nbytes,
                     round_ms=[round(x, 4) for x in per[v]], best_ms=round(best, 4),
                     gbs=round(2 * nbytes / best / 1e6, 1), of_copy=round(ceil / best, 3))
            del keys, part, src, dst, ref
        elif name == "world1":
            from distml_amd.group import NativeShardGroup
            rows, cols = 1_250_000, 200
            grp = NativeShardGroup(DataDesc(1, 0, 1), rows, cols, 0, 1, NativeShardGroup.unique_id())
            grp.store.synth_fill(7)
            rec = 4 + 4 * cols
            keys = torch.randint(0, rows, (rows,), dtype=torch.int64, device="cuda", generator=g)
            nbytes = rows * rec
            out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            ref = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def fetch():
                ln = C.c_int64()
                t0 = time.perf_counter()
                assert L.dml_store_fetch_device(grp.store._h, C.c_void_p(keys.data_ptr()), rows, C.c_void_p(ref.data_ptr()),
                                                nbytes, C.byref(ln), None) == 0
                return (time.perf_counter() - t0) * 1e3

            def pull(order):
                t0 = time.perf_counter()
                assert grp.pull(keys.data_ptr(), rows, out.data_ptr(), nbytes, request_order=order)[0] == nbytes
                return (time.perf_counter() - t0) * 1e3

            fetch()
            pull(False)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), "world 1: the pull's bytes are the fetch's"
            per = rounds([("dml_store_fetch_device", fetch), ("dml_group_pull", lambda: pull(False)),
                          ("dml_group_pull/request-order", lambda: pull(True))], args.rounds, args.calls)
            base = min(per["dml_store_fetch_device"])
            for v in per:
                best = min(per[v])
                emit(shape=name, rows=rows, cols=cols, keys=rows, variant=v, out_bytes=nbytes,
                     round_ms=[round(x, 4) for x in per[v]], best_ms=round(best, 4),
                     gbs=round(2 * nbytes / best / 1e6, 1), of_fetch=round(base / best, 3))
            grp.close()
            del keys, out, ref
        else:
            raise SystemExit(f"unknown shape {name}")
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

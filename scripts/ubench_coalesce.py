#!/usr/bin/env python3
"""Timing of the device gradient coalescer: the three stages of
dml_coalesce_device (order: k_co_pairs and the radix sort; heads: k_co_heads twice and
k_co_offsets; sum: k_co_sum), taken from the call's own HIP events (dml_diag_coalesce_times),
against the box's plain copy of the sum's bytes (dml_diag_stream, copy = 1, over
(n x row + m x row) / 2 bytes, so it reads and writes n x row + m x row together) in the same
process. torch's index_add_ on the same inputs (inverse precomputed) is timed beside them for
context only: its adds are atomic, so its sums are unordered and it is no yardstick.

Per shape every candidate is warmed up, the coalescer's output is compared between two runs,
then --rounds rounds alternate the candidates; a round's figure is the median of --calls calls.
One JSON line per shape goes to --out (default profiles/coalesce_ubench.jsonl).

Shapes: 200 f32 columns at n = 2^20 occurrences with (distinct) every key once, (x4) four
occurrences per key, (zipf) a Zipf(1.1) list, (half) one key holding half the list; and
(arr) cols = 1 at n = 2^24, four occurrences per key on average.

  python scripts/ubench_coalesce.py [--shapes distinct,x4,zipf,half,arr] [--calls 5] [--rounds 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("distinct", "x4", "zipf", "half", "arr")


def make_keys(name, rng, np):
    n = 1 << 24 if name == "arr" else 1 << 20
    if name == "distinct":
        k = rng.permutation(n)
    elif name == "x4":
        k = rng.permutation(n) >> 2
    elif name == "zipf":
        k = np.minimum(rng.zipf(1.1, size=n), 1 << 20)
    elif name == "half":
        k = rng.permutation(n)
        k[rng.permutation(n)[: n // 2]] = 7
    else:
        k = rng.integers(0, n >> 2, size=n)
    return k.astype(np.int64), (1 if name == "arr" else 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coalesce_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DeviceKeys, _lib
    assert torch.cuda.is_available(), "ubench_coalesce needs the GPU"
    L = _lib.load()
    lines = []
    for name in args.shapes.split(","):
        rng = np.random.default_rng(5)
        keys, cols = make_keys(name, rng, np)
        n, row = len(keys), 4 * cols
        fmt = DataDesc(1 if cols > 1 else 0, 1, 1, False, True, False)
        uk, counts = np.unique(keys, return_counts=True)
        m = len(uk)
        moved = (n + m) * row
        dk = torch.from_numpy(keys).cuda()
        vals = torch.randn((n, cols), dtype=torch.float32, device="cuda")
        kout = torch.empty(m, dtype=torch.int64, device="cuda")
        vout = torch.empty((m, cols), dtype=torch.float32, device="cuda")
        inv = torch.empty(n, dtype=torch.int32, device="cuda")
        half = (moved // 2 + 15) & ~15
        src = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        co = Coalescer(0)
        torch.cuda.synchronize()

        def coalesce():
            assert co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), vals.data_ptr(), kout.data_ptr(), vout.data_ptr(),
                          inv.data_ptr(), m, stream=st.cuda_stream) == m
            return co.stage_times()

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), half, C.c_void_p(st.cuda_stream),
                                     C.byref(ms)) == 0
            return ms.value

        def index_add():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                acc.zero_()
                acc.index_add_(0, inv64, vals)
                e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        coalesce()
        first = vout.clone()
        coalesce()
        assert torch.equal(first.view(torch.int32), vout.view(torch.int32)), name  # run to run, bit for bit
        assert torch.equal(kout.cpu(), torch.from_numpy(uk))
        del first
        inv64 = inv.long()
        acc = torch.empty((m, cols), dtype=torch.float32, device="cuda")
        copy()
        index_add()
        per = dict(order=[], heads=[], sum=[], copy=[], index_add=[])
        for _ in range(args.rounds):
            t = [coalesce() for _ in range(args.calls)]
            for i, k in enumerate(("order", "heads", "sum")):
                per[k].append(statistics.median(x[i] for x in t))
            per["copy"].append(statistics.median(copy() for _ in range(args.calls)))
            per["index_add"].append(statistics.median(index_add() for _ in range(args.calls)))
        best = {k: min(v) for k, v in per.items()}
        ln = dict(shape=name, n=n, m=m, cols=cols, row_bytes=row, longest_segment=int(counts.max()),
                  sum_moved_bytes=moved, round_ms={k: [round(x, 4) for x in v] for k, v in per.items()},
                  best_ms={k: round(v, 4) for k, v in best.items()},
                  sum_gbs=round(moved / best["sum"] / 1e6, 1), copy_gbs=round(2 * half / best["copy"] / 1e6, 1),
                  sum_over_copy=round(best["sum"] / best["copy"], 3),
                  index_add_over_sum=round(best["index_add"] / best["sum"], 3))
        lines.append(ln)
        print(json.dumps(ln), flush=True)
        co.close()
        del dk, vals, kout, vout, inv, inv64, acc, src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

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

The sum is timed twice where the library has the threshold (dml_coalescer_set_long_min): `sum`
with --long-min (0: the default DML_COALESCE_LONG_MIN), `sum_walk` with the threshold at never,
so that the walk and the long-segment kernels are compared in one process; `call` is the three
stages of the first together. --lib loads another build of the library (an older one without
the threshold reports `sum` only), for A/B runs in alternating processes.

Shapes: 200 f32 columns at n = 2^20 occurrences with (distinct) every key once, (x4) four
occurrences per key, (zipf) a Zipf(1.1) list, (half) one key holding half the list; and
(arr) cols = 1 at n = 2^24, four occurrences per key on average. The threshold sweep: (seg:L)
200 f32 columns at n = 2^18, all distinct but one key that holds L occurrences, and (aseg:L)
the same at cols = 1; without --long-min their threshold is L, so that segment alone is long.

--packed times dml_coalesce_pack_device's sum stage (`fused`, where the loaded library has the
call) beside the two calls it replaces on the same inputs: dml_coalesce_device's `sum` stage
and k_rec_pack (`pack`, HIP events around dml_records_pack_device). Run it once on this build
and once with --lib (and --label parent) on the parent's, in alternating processes: the parent's `sum` + `pack` is
the yardstick of `fused`, and the two builds' `sum` show whether the dense form moved.
--expand times dml_records_expand_device at 200 f32 columns and AdaGrad 200 (both planes),
n = 2^20, over the distinct, x4 and zipf lists, beside the plain copy of its
m x F + n x row bytes and k_rec_unpack plus torch's gather. Both write to
profiles/coalesce_pack_ubench.jsonl unless --out says otherwise (appending).
--elems times dml_coalesce_elems_device (see bench_elems) into profiles/coalesce_elems_ubench.jsonl.
--key-range FIRST:LAST (or `auto`: the list's smallest key to its largest) declares the range
(dml_coalescer_set_key_range), so that `order` is the bounded stage's time; the
line then holds the route (dml_diag_coalesce_order) and, for context only, `torch_sort`:
torch.sort(stable=True) of the int32 relative keys. Its yardstick is `order` of the parent's
library (--lib, --label parent) in alternating processes, every process with --append and
--out profiles/coalesce_order_ubench.jsonl.

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
ELEMS_SHAPES = ("uniform", "zipf", "half", "narrow", "seg:128", "seg:256", "seg:512", "seg:1024", "seg:4096")


def make_keys(name, rng, np):
    n = 1 << 24 if name == "arr" else 1 << 18 if "seg:" in name else 1 << 20
    if "seg:" in name:
        k = rng.permutation(n) + 8
        k[rng.permutation(n)[: int(name.split(":")[1])]] = 7
        return k.astype(np.int64), (1 if name[0] == "a" else 200)
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


def timed(st, fn):
    """Milliseconds of what fn enqueues on stream st, by HIP events."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def rounds_of(cands, rounds, calls):
    """{name: [per round, the median of `calls` calls]} with the candidates alternating."""
    per = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    names = list(cands)
    for r in range(rounds):  # each round starts one candidate later: none always follows the same one
        for k in names[r % len(names):] + names[:r % len(names)]:
            per[k].append(statistics.median(cands[k]() for _ in range(calls)))
    return per


def emit(ln, per, out):
    ln["round_ms"] = {k: [round(x, 4) for x in v] for k, v in per.items()}
    ln["best_ms"] = {k: round(min(v), 4) for k, v in per.items()}
    print(json.dumps(ln), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(json.dumps(ln) + "\n")


def bench_packed(args, np, torch):
    from distml_amd import Coalescer, DataDesc, DeviceKeys, _lib, pack_push_device, record_bytes
    fused = "dml_coalesce_pack_device" in _lib.SIGNATURES
    for name in args.shapes.split(","):
        keys, cols = make_keys(name, np.random.default_rng(5), np)
        n, m = len(keys), len(np.unique(keys))
        fmt = DataDesc(1 if cols > 1 else 0, 1, 1, False, True, False)
        R = record_bytes(fmt, cols)[0]
        dk = torch.from_numpy(keys).cuda()
        vals = torch.randn((n, cols), dtype=torch.float32, device="cuda")
        kout = torch.empty(m, dtype=torch.int64, device="cuda")
        vout = torch.empty((m, cols), dtype=torch.float32, device="cuda")
        rec2 = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        rec1 = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        co = Coalescer(0)
        if args.long_min:
            co.set_long_min(args.long_min)
        torch.cuda.synchronize()

        def dense():
            co.run(fmt, cols, DeviceKeys(dk.data_ptr(), n), vals.data_ptr(), kout.data_ptr(), vout.data_ptr(), None, m,
                   stream=st.cuda_stream)
            return co.stage_times()[2]

        def pack():
            return timed(st, lambda: pack_push_device(fmt, cols, DeviceKeys(kout.data_ptr(), m), vout.data_ptr(), m,
                                                      rec2.data_ptr(), m * R, stream=st.cuda_stream))

        def packed():
            co.run_packed(fmt, cols, DeviceKeys(dk.data_ptr(), n), vals.data_ptr(), rec1.data_ptr(), m * R,
                          stream=st.cuda_stream)
            return co.stage_times()[2]

        cands = dict(sum=dense, pack=pack)
        if fused:
            cands["fused"] = packed
        per = rounds_of(cands, args.rounds, args.calls)
        if fused:
            torch.cuda.synchronize()
            assert torch.equal(rec1, rec2), name  # the fused bytes are the two calls'
        emit(dict(mode="packed", lib=args.label, shape=name, n=n, m=m, cols=cols, record_bytes=R,
                  two_call_bytes=(n + m) * 4 * cols + m * (4 * cols + R), fused_bytes=n * 4 * cols + m * R), per, args.out)
        co.close()
        del dk, vals, kout, vout, rec1, rec2
        torch.cuda.empty_cache()


def bench_expand(args, np, torch):
    from distml_amd import DataDesc, _lib, expand_fetch_device, record_bytes, unpack_fetch_device
    L = _lib.load()
    for ada in (False, True):
        for name in ("distinct", "x4", "zipf"):
            keys, cols = make_keys(name, np.random.default_rng(5), np)
            uk, hinv = np.unique(keys, return_inverse=True)
            n, m = len(keys), len(uk)
            fmt = DataDesc(1, 1, 1, False, True, ada)
            F = record_bytes(fmt, cols)[1]
            planes = 2 if ada else 1
            moved = m * F + planes * n * 4 * cols
            rec = torch.randint(0, 1 << 31, (m * F // 4,), dtype=torch.int32, device="cuda")
            inv = torch.from_numpy(hinv.reshape(-1).astype(np.int32)).cuda()
            inv64 = inv.long()
            occ = [torch.empty((n, cols), dtype=torch.float32, device="cuda") for _ in range(planes)]
            uni = [torch.empty((m, cols), dtype=torch.float32, device="cuda") for _ in range(planes)]
            half = (moved // 2 + 15) & ~15
            src = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1)
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            st = torch.cuda.Stream()
            torch.cuda.synchronize()

            def expand():
                return timed(st, lambda: expand_fetch_device(fmt, cols, rec.data_ptr(), m, inv.data_ptr(), n,
                                                             occ[0].data_ptr(), occ[1].data_ptr() if ada else None,
                                                             stream=st.cuda_stream))

            def copy():
                ms = C.c_float()
                assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), half, C.c_void_p(st.cuda_stream),
                                         C.byref(ms)) == 0
                return ms.value

            def unpack_gather():
                def go():
                    unpack_fetch_device(fmt, cols, rec.data_ptr(), m, uni[0].data_ptr(),
                                        uni[1].data_ptr() if ada else None, None, stream=st.cuda_stream)
                    with torch.cuda.stream(st):
                        for u, o in zip(uni, occ2):
                            torch.index_select(u, 0, inv64, out=o)
                return timed(st, go)

            occ2 = [torch.empty_like(o) for o in occ]
            per = rounds_of(dict(expand=expand, copy=copy, unpack_gather=unpack_gather), args.rounds, args.calls)
            torch.cuda.synchronize()
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(occ, occ2)), name
            ln = dict(mode="expand", shape=name, ada=ada, n=n, m=m, cols=cols, fetch_record_bytes=F, moved_bytes=moved)
            emit(ln, per, args.out)
            del rec, inv, inv64, occ, occ2, uni, src, dst
            torch.cuda.empty_cache()


def bench_elems(args, np, torch):
    """dml_coalesce_elems_device, record form, per_occ = 2 (a LightLDA move).
    Shapes: uniform / zipf / half at 1 000 columns and narrow at 64, n = 2^20 tokens; seg:L, one
    key of L tokens among 2^18 distinct ones. `sum` is the call's sum stage at --long-min (seg:L:
    at L), `sum_short` with the threshold at never, `call` its three stages, `order` the sort's;
    `copy` the plain copy of the n x per_occ x 8 + m x R bytes the stage must move; `index_put`
    today's route on the same inputs (zeroed plane, index_put_(accumulate=True) with the inverse
    given, pack_push_device); `onehot` run_packed's sum stage fed one one-hot-pair row per token."""
    from distml_amd import Coalescer, DataDesc, DeviceKeys, _lib, pack_push_device, record_bytes
    L, per_occ, NEVER = _lib.load(), 2, 1 << 31
    for name in args.shapes.split(","):
        rng = np.random.default_rng(5)
        if "seg:" in name:
            keys, cols = make_keys(name, rng, np)[0], 1000
        else:
            n = 1 << 20
            cols = 64 if name == "narrow" else 1000
            keys = (np.minimum(rng.zipf(1.1, size=n), 1 << 20) if name == "zipf" else rng.integers(0, 65536, size=n)).astype(np.int64)
            if name == "half":
                keys[rng.permutation(n)[: n // 2]] = 7
        n = len(keys)
        uk, hinv = np.unique(keys, return_inverse=True)
        m = len(uk)
        fmt = DataDesc(1, 0, 0, False, True, False)
        R = record_bytes(fmt, cols)[0]
        moved = n * per_occ * 8 + m * R
        dk = torch.from_numpy(keys).cuda()
        dc = torch.from_numpy(rng.integers(0, cols, size=(n, per_occ)).astype(np.int32)).cuda()
        dv = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
        rec1 = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        rec2 = torch.empty_like(rec1)
        plane = torch.empty((m, cols), dtype=torch.int32, device="cuda")
        ukd = torch.from_numpy(uk).cuda()
        rows64 = torch.from_numpy(hinv.reshape(-1)).cuda().long()[:, None].expand(n, per_occ)
        cols64 = dc.long()
        half = (moved // 2 + 15) & ~15
        src = torch.empty(half, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        co = Coalescer(0)
        lm = int(name.split(":")[1]) if "seg:" in name and not args.long_min else args.long_min
        kr = None
        if args.key_range:
            kr = (int(keys.min()), int(keys.max()) + 1) if args.key_range == "auto" else tuple(map(int, args.key_range.split(":")))
            co.set_key_range(*kr)
        torch.cuda.synchronize()

        def elems(long_min=lm, out=rec1):
            co.set_long_min(long_min)
            assert co.run_elems(fmt, cols, DeviceKeys(dk.data_ptr(), n), dc.data_ptr(), dv.data_ptr(), per_occ,
                                out.data_ptr(), m * R, records=True, stream=st.cuda_stream) == (m, m * R)
            return co.stage_times()

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), half, C.c_void_p(st.cuda_stream), C.byref(ms)) == 0
            return ms.value

        def index_put():
            def go():
                with torch.cuda.stream(st):
                    plane.zero_()
                    plane.index_put_((rows64, cols64), dv, accumulate=True)
                pack_push_device(fmt, cols, DeviceKeys(ukd.data_ptr(), m), plane.data_ptr(), m, rec2.data_ptr(), m * R,
                                 stream=st.cuda_stream)
            return timed(st, go)

        cands = dict(sum=lambda: elems()[2], sum_short=lambda: elems(NEVER)[2], call=lambda: sum(elems()),
                     order=lambda: elems()[0], copy=copy, index_put=index_put)
        hot = None
        if "seg:" not in name:  # the n x cols one-hot plane: 4 GiB at 1 000 columns
            hot = torch.zeros((n, cols), dtype=torch.int32, device="cuda")
            hot.index_put_((torch.arange(n, device="cuda")[:, None].expand(n, per_occ), cols64), dv, accumulate=True)

            def onehot():
                co.set_long_min(0)
                co.run_packed(fmt, cols, DeviceKeys(dk.data_ptr(), n), hot.data_ptr(), rec2.data_ptr(), m * R,
                              stream=st.cuda_stream)
                return co.stage_times()[2]
            cands["onehot"] = onehot
        elems()
        route = co.route()
        index_put()
        torch.cuda.synchronize()
        assert torch.equal(rec1, rec2), name  # today's route writes the same bytes
        elems(NEVER, rec2)
        torch.cuda.synchronize()
        assert torch.equal(rec1, rec2), name  # and so does the short route
        per = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per.items()}
        emit(dict(mode="elems", lib=args.label, key_range=kr, order_route=co.order_route() if kr else None, shape=name, n=n, m=m, cols=cols, per_occ=per_occ, record_bytes=R, long_min=lm, route=route,
                  longest_segment=int(np.bincount(hinv.reshape(-1)).max()), sum_moved_bytes=moved,
                  sum_over_copy=round(best["sum"] / best["copy"], 3), index_put_over_sum=round(best["index_put"] / best["sum"], 3)),
             per, args.out)
        co.close()
        del dk, dc, dv, rec1, rec2, plane, rows64, cols64, src, dst, hot
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--long-min", type=int, default=0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="this", help="the `lib` field of --packed's lines")
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--expand", action="store_true")
    ap.add_argument("--elems", action="store_true")
    ap.add_argument("--key-range", default=None, help="FIRST:LAST or auto")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "coalesce_elems_ubench.jsonl" if args.elems else
                                        "coalesce_pack_ubench.jsonl" if args.packed or args.expand else "coalesce_ubench.jsonl")
    if args.elems and args.shapes == ",".join(SHAPES):
        args.shapes = ",".join(ELEMS_SHAPES)
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DeviceKeys, _lib
    assert torch.cuda.is_available(), "ubench_coalesce needs the GPU"
    if args.lib:
        raw = C.CDLL(args.lib)
        for sym in [s for s in _lib.SIGNATURES if not hasattr(raw, s)]:
            del _lib.SIGNATURES[sym]
        _lib._lib = _lib.load(args.lib)
    if args.packed or args.expand or args.elems:
        (bench_elems if args.elems else bench_packed if args.packed else bench_expand)(args, np, torch)
        return
    L = _lib.load()
    knob = "dml_coalescer_set_long_min" in _lib.SIGNATURES
    NEVER = 1 << 31
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
        kr = None
        if args.key_range:
            kr = (int(keys.min()), int(keys.max()) + 1) if args.key_range == "auto" else tuple(map(int, args.key_range.split(":")))
            co.set_key_range(*kr)
            rel = (dk - kr[0]).to(torch.int32)
        torch.cuda.synchronize()

        lm = int(name.split(":")[1]) if "seg:" in name and not args.long_min else args.long_min

        def coalesce(long_min=lm):
            if knob:
                co.set_long_min(long_min)
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
        route = co.route() if knob else None
        if knob:
            coalesce(NEVER)
            assert torch.equal(first.view(torch.int32), vout.view(torch.int32)), name  # walk and long, bit for bit
        assert torch.equal(kout.cpu(), torch.from_numpy(uk))
        del first
        inv64 = inv.long()
        acc = torch.empty((m, cols), dtype=torch.float32, device="cuda")
        copy()
        index_add()
        per = dict(order=[], heads=[], sum=[], call=[], copy=[], index_add=[])
        if knob:
            per["sum_walk"] = []
        if kr:
            per["torch_sort"] = []
        for _ in range(args.rounds):
            t = [coalesce() for _ in range(args.calls)]
            for i, k in enumerate(("order", "heads", "sum")):
                per[k].append(statistics.median(x[i] for x in t))
            per["call"].append(statistics.median(sum(x) for x in t))
            if knob:
                per["sum_walk"].append(statistics.median(coalesce(NEVER)[2] for _ in range(args.calls)))
            per["copy"].append(statistics.median(copy() for _ in range(args.calls)))
            per["index_add"].append(statistics.median(index_add() for _ in range(args.calls)))
            if kr:
                with torch.cuda.stream(st):
                    per["torch_sort"].append(statistics.median(timed(st, lambda: torch.sort(rel, stable=True))
                                                               for _ in range(args.calls)))
        best = {k: min(v) for k, v in per.items()}
        ln = dict(shape=name, n=n, m=m, cols=cols, row_bytes=row, longest_segment=int(counts.max()),
                  long_min=lm, route=route, lib=args.label, key_range=kr, order_route=co.order_route() if kr else None,
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
    with open(args.out, "a" if args.append else "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

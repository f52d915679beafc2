#!/usr/bin/env python3
"""Timing of the device record codec: k_rec_pack and k_rec_unpack with
each of their load paths (DML_CODEC_KNOB_LOADS 1 = every dword gathered singly, 2 = 16-byte
loads; 0 = the shipped choice by record length) against the box's plain copy of the same
bytes (dml_diag_stream, copy = 1, over the record stream's bytes) and against k_fetch_vec's
range form on a store of the same shape, in the same process.

Each call is timed by a pair of HIP events on the stream it runs on. Per shape every
candidate is warmed up, the codec's outputs are compared across the load paths (and pack's
with unpack's inverse where the layouts coincide), then three rounds alternate the
candidates; a round's figure is the median of --calls calls. One JSON line per shape and
candidate goes to --out (default profiles/codec_device.jsonl). `moved` counts the bytes a
candidate reads plus the bytes it writes; gbs = moved / best time.

  python scripts/ubench_codec.py [--shapes cfg2,cfg4,cfg4ada,arr3,arr2[,w64,...]] [--calls 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (data type, key type, value type, AdaGrad, records, cols)
SHAPES = {
    "cfg2": (1, 0, 1, False, 16_384, 1024),        # 1 025-dword records
    "cfg4": (1, 0, 1, False, 1_250_000, 200),      # 201
    "cfg4ada": (1, 0, 1, True, 1_250_000, 200),    # fetch record 401 (the push record is cfg4's)
    "arr3": (0, 0, 3, False, 1_000_000, 1),        # 3 (f64 behind an int32 key)
    "arr2": (0, 0, 0, False, 1_000_000, 1),        # 2
    # not in the default set: record lengths for the load-path thresholds
    "w16": (1, 0, 1, False, 4_000_000, 16),
    "w64": (1, 0, 1, False, 2_000_000, 64),
    "w96": (1, 0, 1, False, 1_500_000, 96),
    "w128": (1, 0, 1, False, 1_000_000, 128),
    "w256": (1, 0, 1, False, 1_000_000, 256),
    "w320": (1, 0, 1, False, 800_000, 320),
    "w512": (1, 0, 1, False, 500_000, 512),
    "w768": (1, 0, 1, False, 330_000, 768),
    "ada8": (1, 0, 1, True, 4_000_000, 8),
    "ada16": (1, 0, 1, True, 4_000_000, 16),
    "ada32": (1, 0, 1, True, 2_000_000, 32),
    "ada64": (1, 0, 1, True, 2_000_000, 64),
    "ada128": (1, 0, 1, True, 1_000_000, 128),
    "ada512": (1, 0, 1, True, 300_000, 512),
}
DEFAULT = "cfg2,cfg4,cfg4ada,arr3,arr2"
LOADS = (("gather", 1), ("16-byte-loads", 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_device.jsonl"))
    args = ap.parse_args()
    import torch
    from distml_amd import (DataDesc, DataStore, KeyRange, _lib, pack_push_device, record_bytes,
                            unpack_fetch_device)
    assert torch.cuda.is_available(), "ubench_codec needs the GPU"
    L = _lib.load()
    lines = []
    for name in args.shapes.split(","):
        dt, kt, vt, ada, n, cols = SHAPES[name]
        fmt = DataDesc(dt, kt, vt, False, True, ada)
        V = 8 if vt == 3 else 4
        push_rec, fetch_rec = record_bytes(fmt, cols)
        plane = n * cols * V
        s = DataStore(fmt, KeyRange(0, n - 1), cols)
        if ada:
            s.setAlpha(0.025, 0.0001, 1.5)
        s.synth_fill(7)
        sst = torch.cuda.ExternalStream(s.stream())
        st = torch.cuda.Stream()
        recs = torch.empty(n * fetch_rec + 16, dtype=torch.uint8, device="cuda")     # the fetched stream
        packed = torch.empty(n * push_rec + 16, dtype=torch.uint8, device="cuda")
        vals = torch.empty(plane + 16, dtype=torch.uint8, device="cuda")
        alpha = torch.empty(n * cols * 4 + 16, dtype=torch.uint8, device="cuda") if ada else None
        ref = torch.empty(n * fetch_rec + 16 & ~15, dtype=torch.uint8, device="cuda")
        src = torch.empty(n * fetch_rec + 16 & ~15, dtype=torch.uint8, device="cuda").fill_(1)
        torch.cuda.synchronize()

        def timed(stream, f):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def fetch_vec():
            return timed(sst, lambda: s.handleFetchDevice(fmt, KeyRange(0, n - 1), recs.data_ptr(), n * fetch_rec,
                                                          stream=sst.cuda_stream))

        def pack(loads):
            L.dml_diag_codec_knob(_lib.DML_CODEC_KNOB_LOADS, loads)
            return timed(st, lambda: pack_push_device(fmt, cols, 0, vals.data_ptr(), n, packed.data_ptr(), n * push_rec,
                                                      stream=st.cuda_stream))

        def unpack(loads, with_alpha):
            L.dml_diag_codec_knob(_lib.DML_CODEC_KNOB_LOADS, loads)
            return timed(st, lambda: unpack_fetch_device(fmt, cols, recs.data_ptr(), n, vals.data_ptr(),
                                                         alpha.data_ptr() if with_alpha else None, None,
                                                         stream=st.cuda_stream))

        def copy(nbytes):
            ms = C.c_float()
            assert L.dml_diag_stream(1, ref.data_ptr(), src.data_ptr(), nbytes & ~15, C.c_void_p(st.cuda_stream),
                                     C.byref(ms)) == 0
            return ms.value

        # candidate -> (callable, bytes read + written, the copy it is compared with)
        runs = {"k_fetch_vec/range": (fetch_vec, n * fetch_rec + plane * (2 if ada else 1), "copy/fetch-stream")}
        for tag, k in LOADS + (("shipped", 0),):
            runs[f"pack/{tag}"] = ((lambda k=k: pack(k)), n * push_rec + plane, "copy/push-stream")
            runs[f"unpack/{tag}"] = ((lambda k=k: unpack(k, False)), n * fetch_rec + plane, "copy/fetch-stream")
            if ada:
                runs[f"unpack+alpha/{tag}"] = ((lambda k=k: unpack(k, True)), 2 * n * fetch_rec + 2 * plane,
                                               "copy/fetch-stream")
        runs["copy/push-stream"] = ((lambda: copy(n * push_rec)), 2 * (n * push_rec & ~15), None)
        runs["copy/fetch-stream"] = ((lambda: copy(n * fetch_rec)), 2 * (n * fetch_rec & ~15), None)

        # warm-up, and the same bytes from every load path
        for _ in range(3):
            fetch_vec()
        torch.cuda.synchronize()
        outs = {}
        for tag, k in LOADS + (("shipped", 0),):
            for _ in range(2):
                unpack(k, ada)
                pack(k)
            torch.cuda.synchronize()
            outs[tag] = (vals.clone(), packed.clone(), alpha.clone() if ada else None)
        base = outs["gather"]
        for tag, o in outs.items():
            assert torch.equal(o[0][:plane], base[0][:plane]) and torch.equal(o[1][:n * push_rec], base[1][:n * push_rec]), \
                (name, tag)
            assert not ada or torch.equal(o[2][:n * cols * 4], base[2][:n * cols * 4]), (name, tag)
        if push_rec == fetch_rec and not ada:  # pack(unpack(stream)) is the stream, up to the keys (0 .. n-1 both)
            assert torch.equal(base[1][:n * push_rec], recs[:n * push_rec]), name
        del outs, base
        for f, _, _ in runs.values():
            f()
        per = {v: [] for v in runs}
        for _ in range(args.rounds):
            for v, (f, _, _) in runs.items():
                per[v].append(statistics.median(f() for _ in range(args.calls)))
        L.dml_diag_codec_knob(_lib.DML_CODEC_KNOB_LOADS, 0)
        for v, (_, moved, against) in runs.items():
            best = min(per[v])
            ln = dict(shape=name, records=n, cols=cols, adagrad=ada, push_rec_dw=push_rec // 4,
                      fetch_rec_dw=fetch_rec // 4, candidate=v, moved_bytes=moved,
                      round_ms=[round(x, 4) for x in per[v]], best_ms=round(best, 4),
                      gbs=round(moved / best / 1e6, 1))
            if against:
                ln["of_copy"] = round(min(per[against]) / best, 3)
                ln["of_fetch_vec"] = round(min(per["k_fetch_vec/range"]) / best, 3)
            lines.append(ln)
            print(json.dumps(ln), flush=True)
        s.close()
        del recs, packed, vals, alpha, ref, src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

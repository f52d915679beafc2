#!/usr/bin/env python3
"""A/B of the device fetch's encode kernels: k_fetch (DML_KNOB_FETCH_KERNEL
1, the host fetch's kernel) against k_fetch_vec (2, and its other launch shapes) and against
the box's plain-copy ceiling (dml_diag_stream, copy = 1) over the same number of output bytes.

Each fetch is timed by a pair of HIP events on the store's apply stream, the stream the
encode runs on (for a key list the pair also spans the one-thread verdict kernel and its
16-byte copy home). Per shape: every variant is warmed up, its output is compared with
k_fetch's at the timed size, then three rounds alternate the variants in one process;
a round's figure is the median of --calls fetches. One JSON line per shape and variant goes
to --out (default profiles/fetch_device.jsonl); rates count the output bytes once read and
once written (2 x out_bytes), as the copy ceiling's do.

  python scripts/ubench_fetch.py [--shapes cfg2,cfg4,cfg4ada,cfg5,array[,w256,w384,w512,w768]] [--calls 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOB = 3
VARIANTS = [("k_fetch", 1), ("k_fetch_vec", 2), ("k_fetch_vec/dword-gather", 2 | 1 << 8),
            ("k_fetch_vec/16-byte-loads", 2 | 2 << 8), ("k_fetch_vec/xcd-order", 2 | 4 << 8),
            ("k_fetch_vec/1-per-thread", 2 | 8 << 8), ("k_fetch_vec/4-per-thread", 2 | 16 << 8)]
# name: (data type, key type, value type, AdaGrad, rows, cols, list length or None for the whole range)
SHAPES = {
    "cfg2": (1, 0, 1, False, 16_384, 1024, None),
    "cfg4": (1, 0, 1, False, 1_250_000, 200, None),
    "cfg4ada": (1, 0, 1, True, 1_250_000, 200, None),
    "cfg5": (1, 0, 0, False, 1_000_000, 1000, 65_536),
    "array": (0, 0, 1, False, 1_000_000_000, 1, 1_000_000),
    # not in the default set: widths between config 4's and config 5's, for the load-path threshold
    "w256": (1, 0, 1, False, 1_000_000, 256, None),
    "w384": (1, 0, 1, False, 650_000, 384, None),
    "w512": (1, 0, 1, False, 500_000, 512, None),
    "w768": (1, 0, 1, False, 330_000, 768, None),
}
DEFAULT = "cfg2,cfg4,cfg4ada,cfg5,array"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_device.jsonl"))
    args = ap.parse_args()
    import torch
    from distml_amd import DataDesc, DataStore, DeviceKeys, KeyRange, _lib
    assert torch.cuda.is_available(), "ubench_fetch needs the GPU"
    L = _lib.load()
    lines = []
    for name in args.shapes.split(","):
        dt, kt, vt, ada, rows, cols, nlist = SHAPES[name]
        s = DataStore(DataDesc(dt, kt, vt, False, True, ada), KeyRange(0, rows - 1), cols)
        if ada:
            s.setAlpha(0.025, 0.0001, 1.5)
        s.synth_fill(7)
        rec = s._fetch_record_bytes()
        if nlist is None:
            what, n = KeyRange(0, rows - 1), rows
        else:
            g = torch.Generator(device="cuda").manual_seed(11)
            keys = torch.randint(0, rows, (nlist,), dtype=torch.int64, device="cuda", generator=g)
            what, n = DeviceKeys(keys.data_ptr(), nlist), nlist
        nbytes = n * rec
        out = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
        ref = torch.empty_like(out)
        src = torch.empty(nbytes + 16 & ~15, dtype=torch.uint8, device="cuda").fill_(1)
        st = torch.cuda.ExternalStream(s.stream())
        torch.cuda.synchronize()

        def one(knob):
            s.set_knob(KNOB, knob)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            assert s.handleFetchDevice(s.format, what, out.data_ptr(), nbytes, stream=st.cuda_stream) == nbytes
            e1.record(st)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, ref.data_ptr(), src.data_ptr(), nbytes & ~15, C.c_void_p(st.cuda_stream),
                                     C.byref(ms)) == 0
            return ms.value

        runs = [(v, (lambda k=k: one(k))) for v, k in VARIANTS] + [("copy", copy)]
        for v, k in VARIANTS:  # warm-up, and the same bytes from every variant at this size
            out.zero_()
            torch.cuda.synchronize()  # torch's stream is not the store's
            for _ in range(3):
                one(k)
            if k == 1:
                ref.copy_(out)
            else:
                assert torch.equal(out, ref), (name, v)
            torch.cuda.synchronize()
        for _ in range(3):
            copy()
        per = {v: [] for v, _ in runs}
        for _ in range(args.rounds):
            for v, f in runs:
                per[v].append(statistics.median(f() for _ in range(args.calls)))
        ceil = min(per["copy"])
        for v, _ in runs:
            best = min(per[v])
            lines.append(dict(shape=name, rows=rows, cols=cols, keys="range" if nlist is None else f"list{nlist}",
                              adagrad=ada, variant=v, out_bytes=nbytes, round_ms=[round(x, 4) for x in per[v]],
                              best_ms=round(best, 4), gbs=round(2 * nbytes / best / 1e6, 1),
                              of_copy=round(ceil / best, 3)))
            print(json.dumps(lines[-1]), flush=True)
        s.close()
        del out, ref, src
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

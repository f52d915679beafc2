"""One rank of the native shard group's chained reduce-scatter
(dml_group_push_chained) in a torch-free process, as the PS JVM runs it;
tests/test_native_chain.py starts `world` of these over the RCCL stand-in
(--double, see tests/native_group_worker.py) or the system RCCL.

Cases (inputs from tests/chain_expect.py, shared with the test's oracle):
  chain   three chained calls back to back, no flush between (the buffer sets
          rotate); call 1: rank 0 passes no push, the others W
  order   chained, push_local of the rank's own rows, chained — no flush between
  fail    world 3, init with -0.0 rows no push lists: rank 1's call 1 hands over
          a push one byte short; every rank makes every call
  jni     GpuShardGroup's nativeGroupPush mode 4 on the mock JNIEnv, the shard
          read back through nativeWriteAll
  unsup   an int32 group: push_chained is refused on every rank, nobody waits
Writes out/<case>_<rank>.npz (the shard's bytes) and prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.modules["torch"] = None  # any `import torch` now raises ImportError
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

from native_group_worker import DOUBLE, Hip, read_uid  # noqa: E402

CALLS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--uid-file", required=True)
    ap.add_argument("--case", required=True)
    ap.add_argument("--vt", type=int, default=1)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--pushes", type=int, default=3)
    ap.add_argument("--pieces", type=int, default=1)
    ap.add_argument("--asc", type=int, default=0)
    ap.add_argument("--out", required=True)
    ap.add_argument("--double", action="store_true")
    a = ap.parse_args()
    dbl = C.CDLL(DOUBLE, mode=C.RTLD_GLOBAL) if a.double else None  # before libdistml_ps.so
    from distml_amd import DataDesc, _lib
    from distml_amd.group import NativeShardGroup
    import pyoracle
    import chain_expect as X
    _lib.load()
    H = Hip(a.device)
    uid = read_uid(a.uid_file, a.rank)
    world, rank, rows, cols, W = a.world, a.rank, a.rows, a.cols, a.pushes
    errors, res = [], {}
    first, last = X.shard_ranges(world, rows)[rank]

    def chained(g, bufs, lens=None):
        ptrs = [H.put(b) for b in bufs]
        g.push_chained(ptrs, lens if lens is not None else [b.nbytes for b in bufs])

    if a.case in ("chain", "order", "fail"):
        vt = a.vt
        g = NativeShardGroup(DataDesc(1, 0, vt), rows, cols, rank, world, uid, device=a.device, pieces=a.pieces)
        init = X.minus_zero_init(vt, rows, cols) if a.case == "fail" else X.init_values(vt, rows, cols)
        g.store.load_values(init[first:last + 1])
        if a.case == "chain":
            calls = X.chain_calls(pyoracle, vt, world, rows, cols, W, CALLS, asc=bool(a.asc),
                                  short=lambda r, c: (r, c) == (0, 1))
            for c in range(CALLS):
                try:
                    chained(g, calls[c][rank])
                except Exception as e:
                    errors.append([c, type(e).__name__, str(e)[:200]])
        elif a.case == "order":
            calls = X.chain_calls(pyoracle, vt, world, rows, cols, W, 2)
            chained(g, calls[0][rank])
            lp = X.local_push(vt, rank, first, last, cols)
            g.push_local([H.put(lp)], [lp.nbytes])
            chained(g, calls[1][rank])
        else:
            for c in range(CALLS):
                bufs = X.subset_pushes(vt, rank, W, rows, cols, c)
                lens = [b.nbytes for b in bufs]
                if rank == 1 and c == 1:
                    lens[1] -= 1  # not whole records
                try:
                    chained(g, bufs, lens)
                except Exception as e:
                    errors.append([c, type(e).__name__, str(e)[:200]])
        try:
            g.flush()
        except Exception as e:
            errors.append(["flush", type(e).__name__, str(e)[:200]])
        res["data"] = g.store.values().view(np.uint8)
        g.close()
    elif a.case == "unsup":
        g = NativeShardGroup(DataDesc(1, 0, 0), rows, cols, rank, world, uid, device=a.device)
        g.store.load_values(np.zeros((last - first + 1, cols), np.int32))
        bufs = [pyoracle.synth_dense_bucket(0, 0, 0, rows, rows, cols, 5 + rank, 1, 0)]
        try:
            chained(g, bufs)
        except Exception as e:
            errors.append([0, type(e).__name__, getattr(e, "code", None), str(e)[:200]])
        g.flush()
        res["data"] = g.store.values().view(np.uint8)
        g.close()
    elif a.case == "jni":
        from test_jni_shim import MockJVM
        jvm = MockJVM()
        vt = 1
        gh, exc = jvm.call("nativeGroupCreate", jvm.bytes_(uid), world, rank, a.device, 1, 0, vt, 0, 1, 0, rows, cols,
                           a.pieces)
        assert exc is None and gh, exc
        st, exc = jvm.call("nativeGroupStore", gh)
        init = X.init_values(vt, rows, cols)[first:last + 1]
        jvm.call("nativeReadAll", st, jvm.bytes_(init.view("<u4").astype(">u4").tobytes()))
        calls = X.chain_calls(pyoracle, vt, world, rows, cols, W, 2)
        for c in range(2):
            bufs = calls[c][rank]
            _, exc = jvm.call("nativeGroupPush", gh, jvm.longs([H.put(b) for b in bufs]),
                              jvm.longs([b.nbytes for b in bufs]), 4)
            if exc:
                errors.append([c, exc[0], exc[1][:200]])
        _, exc = jvm.call("nativeGroupFlush", gh)
        assert exc is None, exc
        wa, _ = jvm.call("nativeWriteAll", st)
        res["data"] = np.frombuffer(jvm.read(wa), ">u4").astype("<u4").view(np.uint8)
        jvm.call("nativeGroupDestroy", gh)
    else:
        raise SystemExit(f"unknown case {a.case}")
    H.free()
    np.savez(os.path.join(a.out, f"{a.case}_{rank}.npz"), **res)
    calls_n = None
    if dbl is not None:
        dbl.rccl_double_calls.restype = C.c_int64
        calls_n = int(dbl.rccl_double_calls())
    libs = {n: ln.split()[-1] for ln in open("/proc/self/maps") for n in ("librccl", "libdistml_ps") if n in ln}
    print(json.dumps({"rank": rank, "errors": errors, "double_calls": calls_n, "libs": libs}), flush=True)


if __name__ == "__main__":
    main()

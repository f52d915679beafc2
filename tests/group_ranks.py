"""The multi-process harness of the native shard group's GPU tests (test_native_group,
test_native_chain, test_native_chain_ada, test_native_chain_i32) and of their workers.

Test side: run_ranks starts `world` torch-free worker processes, one rank each, and
returns their JSON lines. RCCL refuses two ranks on one GPU, so by default the ranks run
the library's unchanged nccl* calls against tests/rccl_double, a test-only stand-in over
host shared memory that runs every transfer DELAY_US after its inputs are ready (helper
thread, asynchronous to the caller's streams): a stream dependency the library forgets
shows up as wrong bytes.

Worker side: start() bans torch, parses the options every worker shares, loads the
stand-in ahead of libdistml_ps.so and reads the unique id; finish() writes
out/<case>_<rank>.npz and prints the JSON line. This module itself must stay importable
beside torch (the tests import it), so the ban lives in start().
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOUBLE = os.path.join(ROOT, "tests", "rccl_double", "librccl_double.so")
DELAY_US = 20000


def run_ranks(worker, tmp_path, world, case, double=True, delay_us=DELAY_US, no_transfers=(), **kw):
    """Start `world` processes of tests/<worker>, wait for all, return their JSON lines (rank
    order). no_transfers: the cases in which every rank refuses before any send."""
    uid = tmp_path / f"uid_{case}"
    if double:
        # the stand-in's id names its shared-memory segment (rccl_double.cc's format);
        # written here without loading the stand-in, whose HIP runtime (/opt/rocm) must
        # not join torch's in this process
        name = ("dml-rccl-double:/dmlrccl_" + os.urandom(12).hex()).encode()
        uid.write_bytes(name + b"\0" * (128 - len(name)))
    args = [f"--{k.replace('_', '-')}={v}" for k, v in kw.items()]
    env = dict(os.environ, DML_RCCL_DOUBLE_DELAY_US=str(delay_us))
    procs = []
    for r in range(world):
        cmd = [sys.executable, "-u", os.path.join(ROOT, "tests", worker), f"--world={world}", f"--rank={r}",
               f"--uid-file={uid}", f"--case={case}", f"--out={tmp_path}", f"--device={0 if double else r}"] + args
        procs.append(subprocess.Popen(cmd + (["--double"] if double else []), stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, env=env))
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=240)
            assert p.returncode == 0, f"rank {procs.index(p)} rc {p.returncode}:\n{e[-3000:]}"
            outs.append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    print("double_calls", worker, case, world, kw, [d["double_calls"] for d in outs])
    for d in outs:
        assert "libdistml_ps" in d["libs"], d
        if double and world > 1 and case not in no_transfers:
            assert d["double_calls"] > 0, d  # the transfers ran through the stand-in
    return outs


class Hip:
    """hipMalloc / hipMemcpy of the HIP runtime libdistml_ps.so loaded."""

    def __init__(self, device):
        path = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln][0]
        h = C.CDLL(path)
        h.hipSetDevice.argtypes = [C.c_int]
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        assert h.hipSetDevice(device) == 0
        self.h, self.ptrs = h, []

    def put(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), max(arr.nbytes, 1)) == 0
        assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0  # host to device
        self.ptrs.append(p.value)
        return p.value

    def free(self):
        for p in self.ptrs:
            self.h.hipFree(C.c_void_p(p))
        self.ptrs = []


def read_uid(path, rank, timeout=120.0):
    from distml_amd.group import NativeShardGroup
    if rank == 0 and not os.path.exists(path):
        tmp = path + ".tmp"
        with open(tmp, "wb") as f:
            f.write(NativeShardGroup.unique_id())
        os.replace(tmp, path)
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > timeout:
            raise TimeoutError("no unique id from rank 0")
        time.sleep(0.05)
    return open(path, "rb").read()


def start(**defaults):
    """A worker's first call: (options, Hip, unique id). --double: dlopen the stand-in with
    RTLD_GLOBAL before libdistml_ps.so, so the library's nccl* calls resolve to it; without
    it the ranks use the system RCCL, one GPU each. defaults: the worker's own defaults of
    the integer options."""
    sys.modules["torch"] = None  # any `import torch` now raises ImportError
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--uid-file", required=True)
    ap.add_argument("--case", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--double", action="store_true")
    for name, dflt in dict(dict(vt=1, rows=1000, cols=64, pushes=3, pieces=1, asc=0), **defaults).items():
        ap.add_argument(f"--{name}", type=int, default=dflt)
    a = ap.parse_args()
    a.dbl = C.CDLL(DOUBLE, mode=C.RTLD_GLOBAL) if a.double else None
    from distml_amd import _lib
    _lib.load()
    return a, Hip(a.device), read_uid(a.uid_file, a.rank)


def finish(a, H, errors, res):
    """A worker's last call: out/<case>_<rank>.npz and the JSON line (the stand-in's transfer
    count and pinned channel counts, the libraries the process really loaded)."""
    H.free()
    np.savez(os.path.join(a.out, f"{a.case}_{a.rank}.npz"), **res)
    calls, ctas = None, None
    if a.dbl is not None:
        a.dbl.rccl_double_calls.restype = C.c_int64
        calls = int(a.dbl.rccl_double_calls())
        a.dbl.rccl_double_ctas.restype = C.c_int32
        ctas = [int(a.dbl.rccl_double_ctas(0)), int(a.dbl.rccl_double_ctas(1))]
    libs = {n: ln.split()[-1] for ln in open("/proc/self/maps") for n in ("librccl", "libdistml_ps") if n in ln}
    print(json.dumps({"rank": a.rank, "errors": errors, "double_calls": calls, "ctas": ctas, "libs": libs}), flush=True)

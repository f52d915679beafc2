"""One-GPU footprint of the chained reduce-scatter's kernels.

Config 2's geometry: a 16384 x 1024 fp32 model, W ascending full-range pushes.
For N in {4, 8}: the N chain pieces one rank runs in one dml_group_push_chained
call (each S/N rows of the model, base read from a received-slice buffer, output
to a send buffer), timed with the pre-reduce's in-packet events
(dml_prereduce_timing), alternating in one process with one dml_prereduce_piece
over the same pushes and all rows (the reduce-scatter path's per-call kernel).
HBM bytes per call: (W + 2) x S for the chain against (W + 1) x S for the
pre-reduce. The xGMI transfers are not run here: their time is not measured.

After the timed runs the chain pieces' output is compared, on sampled rows, with
the CPU oracle fed base + the pushes in order, byte for byte.

  python scripts/chain_footprint.py --out profiles/chain_footprint.json

runs one child process per W (32 and 4), each under its own `timeout`, and stops
at the first one that fails.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
ROWS, COLS = 16384, 1024


def child(W, reps, warm):
    import numpy as np
    import torch

    import pyoracle
    from distml_amd import DataDesc, _lib
    from distml_amd.group import HipOps
    L = _lib.load()
    ops = HipOps()
    fmt = DataDesc(1, 0, 1)
    rec = 4 + 4 * COLS
    st0 = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty(ROWS * rec, dtype=torch.uint8, device="cuda") for _ in range(W)]
    for b, t in enumerate(bufs):
        assert L.dml_synth_dense_bucket(t.data_ptr(), C.byref(fmt.to_c()), 0, ROWS, ROWS, COLS, 3000 + b, 1, 0,
                                        C.c_void_p(st0)) == 0
    recv = torch.randn(ROWS, COLS, device="cuda")  # the slices as they arrive
    send = torch.empty_like(recv)
    part = torch.empty_like(recv)
    istream, pstream = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ptrs, lens = [t.data_ptr() for t in bufs], [t.numel() for t in bufs]
    L.dml_prereduce_timing(1)

    def timed(run):
        h = ops.begin(fmt, 0, ROWS, COLS, ptrs, lens, istream.cuda_stream)
        run(h)
        pstream.synchronize()
        ops.end(h)
        ms, n = C.c_double(), C.c_int64()
        assert L.dml_prereduce_kernel_time(C.byref(ms), C.byref(n), 1) == 0
        return ms.value, n.value

    def chain(N):
        def run(h):
            per = ROWS // N
            for i in range(N):
                off = i * per * COLS * 4
                ops.chain_piece(h, per, per, i * per, per, recv.data_ptr() + off, send.data_ptr() + off,
                                pstream.cuda_stream)
        return run

    def pre(h):
        ops.piece(h, ROWS, ROWS, 0, ROWS, part.data_ptr(), pstream.cuda_stream)

    out = {"rows": ROWS, "cols": COLS, "pushes": W, "reps": reps, "bytes_ratio": (W + 2) / (W + 1)}
    for N in (4, 8):
        t_chain, t_pre = [], []
        for r in range(warm + reps):
            c, nc = timed(chain(N))
            p, npre = timed(pre)
            assert nc == N and npre == 1, (nc, npre)
            if r >= warm:
                t_chain.append(c)
                t_pre.append(p)
        mc, mp = statistics.median(t_chain), statistics.median(t_pre)
        out[f"N{N}"] = {"chain_ms_median": mc, "chain_ms_min": min(t_chain), "chain_ms_max": max(t_chain),
                        "prereduce_ms_median": mp, "prereduce_ms_min": min(t_pre), "prereduce_ms_max": max(t_pre),
                        "ratio": mc / mp, "ratio_over_bytes_ratio": mc / mp / out["bytes_ratio"]}
    # the timed code is the checked code: sampled rows of the last chain call against the oracle
    rows = np.unique(np.concatenate([np.arange(0, ROWS, 257), [1, ROWS // 8 - 1, ROWS // 8, ROWS - 1]]))
    got = send[torch.from_numpy(rows).cuda()].cpu().numpy()
    o = pyoracle.OracleStore(1, 0, 1, 0, len(rows) - 1, COLS)
    o.data[:] = recv[torch.from_numpy(rows).cuda()].cpu().numpy()
    for b in range(W):
        assert o.push(pyoracle.synth_dense_rows(0, 1, rows, COLS, 3000 + b).tobytes()) == 0
    out["sampled_rows"] = int(len(rows))
    out["sampled_rows_bytes_equal"] = bool(got.view(np.uint32).tobytes() == o.data.view(np.uint32).tobytes())
    out["xgmi_time"] = "not measured"
    print(json.dumps(out), flush=True)
    return 0 if out["sampled_rows_bytes_equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0, help="run the GPU step for this many pushes")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child, a.reps, a.warm))
    res = []
    for W in (32, 4):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), f"--child={W}",
               f"--reps={a.reps}", f"--warm={a.warm}"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(p.returncode)
        res.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"chain_footprint": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""One-GPU footprint of the AdaGrad chain's kernels.

Config 4's geometry cut to fit beside its pushes: a 1.25 M x 200 AdaGrad model, W
ascending full-range pushes (W = 4 and 16). For N in {4, 8}: the N AdaGrad chain
pieces one rank runs in one dml_group_push_chained call (each S/N rows of the
model, data / delta / marks read from a received-slice buffer and written to a
send buffer), timed with the pre-reduce's in-packet events (dml_prereduce_timing),
alternating in one process with the same W pushes applied to one AdaGrad store of
the whole model by dml_store_push_batch_device (dml_store_set_timing: the kernels
the exchange path's owners run, summed over the node; their name and launch count
are recorded). Each call is timed out of place (ring step 0's shape) and in place
(steps 1 .. N-1: the slice is summed where it arrived).
Algorithmic HBM bytes per call, S = one plane: the chain reads W x S + 2 S and
writes 2 S; the store reads 2 S per launch beside the W x S and writes 2-3 S per
launch (alpha where delta is above 1).
The xGMI transfers are not run here: their time, and their overlap with the
pieces, are not measured.

After the timed runs the pieces' data and delta planes are compared, on sampled
rows, with the CPU oracle (ada_grad = 1) fed the base planes + the pushes in order,
byte for byte.

  python scripts/chain_ada_footprint.py --out profiles/chain_ada_footprint.json

runs one child process per W, each under its own `timeout`, and stops at the first
one that fails.
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
ROWS, COLS = 1_250_000, 200


def child(W, reps, warm):
    import numpy as np
    import torch

    import pyoracle
    from distml_amd import DataDesc, DataStore, KeyRange, _lib
    from distml_amd.group import MAXDELTA_RECORD_BYTES, HipOps
    L = _lib.load()
    ops = HipOps()
    fmt = DataDesc(1, 0, 1, False, True, True)
    rec = 4 + 4 * COLS
    st0 = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty(ROWS * rec, dtype=torch.uint8, device="cuda") for _ in range(W)]
    for b, t in enumerate(bufs):
        assert L.dml_synth_dense_bucket(t.data_ptr(), C.byref(fmt.to_c()), 0, ROWS, ROWS, COLS, 3000 + b, 1, 0,
                                        C.c_void_p(st0)) == 0
    recv = [torch.randn(ROWS, COLS, device="cuda"), torch.rand(ROWS, COLS, device="cuda"),
            torch.zeros(ROWS, dtype=torch.int32, device="cuda")]  # the slices as they arrive: data, delta, marks
    send = [torch.empty_like(x) for x in recv]
    record = torch.zeros(MAXDELTA_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    store = DataStore(fmt, KeyRange(0, ROWS - 1), COLS, async_push=True)
    store.set_timing(True)
    istream, pstream = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ptrs, lens = [t.data_ptr() for t in bufs], [t.numel() for t in bufs]
    L.dml_prereduce_timing(1)

    def chain(N, inplace=False):
        h = ops.begin(fmt, 0, ROWS, COLS, ptrs, lens, istream.cuda_stream)
        per = ROWS // N
        dst = recv if inplace else send
        for i in range(N):
            o4, o1 = i * per * COLS * 4, i * per * 4
            ops.chain_piece_ada(h, per, per, i * per, per, recv[0].data_ptr() + o4, recv[1].data_ptr() + o4,
                                recv[2].data_ptr() + o1, dst[0].data_ptr() + o4, dst[1].data_ptr() + o4,
                                dst[2].data_ptr() + o1, record.data_ptr(), True, pstream.cuda_stream)
        pstream.synchronize()
        ops.end(h)
        ms, n = C.c_double(), C.c_int64()
        assert L.dml_prereduce_kernel_time(C.byref(ms), C.byref(n), 1) == 0
        return ms.value, n.value

    def stored():
        store.pushDevice(ptrs, lens)
        store.flush()
        return store.kernel_time()

    out = {"rows": ROWS, "cols": COLS, "pushes": W, "reps": reps, "chain_bytes_S": W + 4}
    for N in (4, 8):
        t_chain, t_in, t_store = [], [], []
        for r in range(warm + reps):
            i, ni = chain(N, inplace=True)  # ring steps 1 .. N-1: the slice is summed where it arrived
            c, nc = chain(N)                # ring step 0's shape: out of place (last: its output is checked below)
            s, ns = stored()
            assert nc == N and ni == N, (nc, ni)
            launches = ns
            if r >= warm:
                t_chain.append(c)
                t_in.append(i)
                t_store.append(s)
        mc, mi, ms = statistics.median(t_chain), statistics.median(t_in), statistics.median(t_store)
        out[f"N{N}"] = {"chain_ms_median": mc, "chain_ms_min": min(t_chain), "chain_ms_max": max(t_chain),
                        "chain_inplace_ms_median": mi, "chain_inplace_ms_min": min(t_in),
                        "chain_inplace_ms_max": max(t_in),
                        "store_ms_median": ms, "store_ms_min": min(t_store), "store_ms_max": max(t_store),
                        "store_launches": launches, "ratio": mc / ms, "ratio_inplace": mi / ms}
    out["store_kernel"] = store.kernel_name()
    # what the store moved: per timed launch data + delta in, data + delta (+ alpha, where delta > 1) out
    out["store_bytes_S"] = [W + 4 * launches, W + 5 * launches]
    out["bytes_ratio"] = [(W + 4) / (W + 5 * launches), (W + 4) / (W + 4 * launches)]
    store.close()
    # the timed code is the checked code: sampled rows of the last chain call against the oracle
    rows = np.unique(np.concatenate([np.arange(0, ROWS, 9973), [1, ROWS // 8 - 1, ROWS // 8, ROWS - 1]]))
    idx = torch.from_numpy(rows).cuda()
    o = pyoracle.OracleStore(1, 0, 1, 0, len(rows) - 1, COLS, ada_grad=1)
    o.data[:] = recv[0][idx].cpu().numpy()
    o.delta[:] = recv[1][idx].cpu().numpy()
    for b in range(W):
        assert o.push(pyoracle.synth_dense_rows(0, 1, rows, COLS, 3000 + b).tobytes()) == 0
    same = all(send[i][idx].cpu().numpy().view(np.uint32).tobytes() == np.ascontiguousarray(w).view(np.uint32).tobytes()
               for i, w in ((0, o.data), (1, o.delta)))
    out["sampled_rows"] = int(len(rows))
    out["sampled_rows_bytes_equal"] = bool(same and bool((send[2][idx] == 1).all()))
    out["xgmi_time"] = "not measured"
    out["xgmi_overlap_with_pieces"] = "not measured"
    print(json.dumps(out), flush=True)
    return 0 if out["sampled_rows_bytes_equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0, help="run the GPU step for this many pushes")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child, a.reps, a.warm))
    res = []
    for W in (16, 4):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), f"--child={W}",
               f"--reps={a.reps}", f"--warm={a.warm}"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(p.returncode)
        res.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"chain_ada_footprint": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""One-GPU footprint of the int32 chain's kernels.

Config 5's geometry: a 1 M x 1 000 int32 model (LightLDA's word-topic counts), W = 32
pushes of 65 536 rows each. For N in {4, 8}: the N ring steps one rank runs in one
dml_group_push_chained_i32 call — per step one chain piece over a slice of S/N rows
(in place, as steps 1 .. N-1 run), the close launch (rollback through the row map)
and the one-wave verdict — timed with the pre-reduce's in-packet events
(dml_prereduce_timing), alternating in one process with
  - the same steps without their close (the close's share when nothing is negative), and
  - the same W pushes applied by dml_store_push_batch_device to one int32 store of the
    whole model (dml_store_set_timing): the yardstick, code this change does not touch.
Algorithmic HBM bytes per call: the chain reads all of S and the pushes and writes all
of S; the store reads and writes only the rows some push lists (`touched`).
The xGMI transfers are not run here: their time, and the cost of sending a slice only
after its verdict, are not measured.

After the timed runs sampled rows of the chain's output are compared with the CPU
oracle (int32) fed the base rows + the pushes that list them, in order, byte for byte,
and the verdict record must still be open.

  python scripts/chain_i32_footprint.py --out profiles/chain_i32_footprint.json

runs the GPU step in a child process under `timeout`.
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
ROWS, COLS, W, NREC = 1_000_000, 1000, 32, 65_536


def perm_a(b):
    return 7919 + 20 * b  # odd, 4 mod 5: coprime to ROWS; another stride per push


def perm_c(b):
    return (b * 31337 + 11) % ROWS


def child(reps, warm):
    import numpy as np
    import torch

    import pyoracle
    from distml_amd import DataDesc, DataStore, KeyRange, _lib
    from distml_amd.group import CHAIN_I32_RECORD_BYTES, HipOps
    L = _lib.load()
    ops = HipOps()
    fmt = DataDesc(1, 0, 0)
    rec = 4 + 4 * COLS
    st0 = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty(NREC * rec, dtype=torch.uint8, device="cuda") for _ in range(W)]
    for b, t in enumerate(bufs):
        assert L.dml_synth_dense_bucket(t.data_ptr(), C.byref(fmt.to_c()), 0, ROWS, NREC, COLS, 5000 + b, perm_a(b),
                                        perm_c(b), C.c_void_p(st0)) == 0
    base = torch.full((ROWS, COLS), 100000, dtype=torch.int32, device="cuda")  # every timed call adds to it again
    keep = base[:: ROWS // 1024].clone()
    record = torch.full((CHAIN_I32_RECORD_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
    store = DataStore(fmt, KeyRange(0, ROWS - 1), COLS, async_push=True)
    ops.assign(store, base.data_ptr(), ROWS * COLS)
    store.flush()
    store.set_timing(True)
    istream, pstream = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ptrs, lens = [t.data_ptr() for t in bufs], [t.numel() for t in bufs]
    L.dml_prereduce_timing(1)
    # rows some push lists
    touched = torch.zeros(ROWS, dtype=torch.bool, device="cuda")
    i = torch.arange(NREC, device="cuda", dtype=torch.int64)
    for b in range(W):
        touched[(perm_a(b) * i + perm_c(b)) % ROWS] = True
    tf = float(touched.float().mean())

    def chain(N, close=True):
        h = ops.begin(fmt, 0, ROWS, COLS, ptrs, lens, istream.cuda_stream)
        per = ROWS // N
        for s in range(N):
            p = base.data_ptr() + s * per * COLS * 4
            ops.chain_piece_i32(h, per, per, s * per, per, p, p, record.data_ptr(), pstream.cuda_stream)
            if close:
                ops.chain_close_i32(h, per, per, s * per, per, p, record.data_ptr(), s, pstream.cuda_stream)
        pstream.synchronize()
        ops.end(h)
        ms, n = C.c_double(), C.c_int64()
        assert L.dml_prereduce_kernel_time(C.byref(ms), C.byref(n), 1) == 0
        return ms.value, n.value

    def stored():
        store.pushDevice(ptrs, lens)
        store.flush()
        return store.kernel_time()

    S = ROWS * COLS * 4
    P = W * NREC * rec
    out = {"rows": ROWS, "cols": COLS, "pushes": W, "rows_per_push": NREC, "reps": reps, "touched_fraction": tf,
           "chain_bytes": 2 * S + P, "store_bytes": 2 * tf * S + P, "bytes_ratio": (2 * S + P) / (2 * tf * S + P)}
    calls = 0
    for N in (4, 8):
        t_chain, t_open, t_store = [], [], []
        for r in range(warm + reps):
            c, nc = chain(N)
            o, no = chain(N, close=False)
            s, ns = stored()
            calls += 2
            assert nc == 2 * N and no == N, (nc, no)
            if r >= warm:
                t_chain.append(c)
                t_open.append(o)
                t_store.append(s)
        mc, mo, ms = statistics.median(t_chain), statistics.median(t_open), statistics.median(t_store)
        out[f"N{N}"] = {"chain_ms_median": mc, "chain_ms_min": min(t_chain), "chain_ms_max": max(t_chain),
                        "pieces_only_ms_median": mo, "pieces_only_ms_min": min(t_open), "pieces_only_ms_max": max(t_open),
                        "store_ms_median": ms, "store_ms_min": min(t_store), "store_ms_max": max(t_store),
                        "store_launches": ns, "ratio": mc / ms, "close_share": (mc - mo) / mc}
    out["store_kernel"] = store.kernel_name()
    store.close()
    # the timed code is the checked code: sampled rows after `calls` chain calls, against the oracle
    rows = np.arange(0, ROWS, ROWS // 1024)
    o = pyoracle.OracleStore(1, 0, 0, 0, len(rows) - 1, COLS)
    o.data[:] = keep.cpu().numpy()
    feeds = []  # per push, the records of the sampled rows it lists (keyed by their place in `rows`)
    for b in range(W):
        listed = ((rows - perm_c(b)) * pow(perm_a(b), -1, ROWS)) % ROWS < NREC
        if listed.any():
            feeds.append(pyoracle.synth_dense_rows(0, 0, rows, COLS, 5000 + b).reshape(len(rows), rec)[listed].tobytes())
    ok = True
    for _ in range(calls):
        for f in feeds:
            ok = ok and o.push(f) == 0
    same = base[:: ROWS // 1024].cpu().numpy().tobytes() == np.ascontiguousarray(o.data).tobytes()
    out["sampled_rows"] = int(len(rows))
    out["sampled_rows_bytes_equal"] = bool(ok and same)
    out["record_open"] = bool((record == 0xFF).all())
    out["xgmi_time"] = "not measured"
    out["late_send_cost"] = "not measured"
    print(json.dumps(out), flush=True)
    return 0 if out["sampled_rows_bytes_equal"] and out["record_open"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=400)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.reps, a.warm))
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child=1",
           f"--reps={a.reps}", f"--warm={a.warm}"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.exit(p.returncode)
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"chain_i32_footprint": res}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

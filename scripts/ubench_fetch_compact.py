#!/usr/bin/env python3
"""Timing of the compact fetch at config 5's geometry: 65 536 distinct words of a
1 M x 1 000 int32 store whose fetched rows hold 1 %, 5 %, 25 % and 100 % non-zero counters (the rows no
key names stay zero and are never read). One process, alternating order (scripts/ubench_coalesce.py's
rounds_of), HIP events on the caller's stream:

  compact         handleFetchCompactRowsDevice: count pass, scan, writing pass;
  count_only      the same call with cap_entries 0: count pass and scan (the writing pass returns at once),
                  so compact - count_only is the writing pass with its second read of the rows;
  records         handleFetchDevice of the same keys (4 004-byte records);
  planes          handleFetchPlanesDevice of the same keys (the dense plane, owner's GPU only);
  compact_expand  compact + expand_compact_rows_device (identity inverse as an int32 list);
  records_expand  records + expand_fetch_device by the same inverse.

Before timing, the expanded compact list is compared with the plane fetch byte for byte.

  python scripts/ubench_fetch_compact.py [--densities 0.01,0.05,0.25,1.0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ubench_coalesce import emit, rounds_of, timed  # noqa: E402

ROWS, WORDS, COLS = 1 << 20, 65536, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--densities", default="0.01,0.05,0.25,1.0")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_compact_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import (DataDesc, DataStore, DeviceKeys, KeyRange, expand_compact_rows_device, expand_fetch_device,
                            pack_push_device, record_bytes)
    assert torch.cuda.is_available(), "ubench_fetch_compact needs the GPU"
    fmt = DataDesc(1, 1, 0, False, True, False)
    Rp, Rf = record_bytes(fmt, COLS)
    rng = np.random.default_rng(5)
    keys = np.sort(rng.choice(ROWS, size=WORDS, replace=False)).astype(np.int64)
    dk = torch.from_numpy(keys).cuda()
    occ = DeviceKeys(dk.data_ptr(), WORDS)
    inv = torch.arange(WORDS, dtype=torch.int32, device="cuda")
    ptr = torch.empty(WORDS + 1, dtype=torch.int32, device="cuda")
    ent = torch.empty((2, WORDS * COLS), dtype=torch.int32, device="cuda")
    recs = torch.empty(WORDS * max(Rp, Rf) // 4, dtype=torch.int32, device="cuda")
    plane = torch.empty((2, WORDS, COLS), dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    for d in (float(x) for x in args.densities.split(",")):
        torch.manual_seed(5)
        vals = torch.randint(1, 1 << 20, (WORDS, COLS), dtype=torch.int32, device="cuda")
        if d < 1.0:
            vals *= torch.rand((WORDS, COLS), device="cuda") < d
        s = DataStore(fmt, KeyRange(0, ROWS - 1), COLS)  # zeros; the named rows take `vals` by one record push
        assert pack_push_device(fmt, COLS, occ, vals.data_ptr(), WORDS, recs.data_ptr(), WORDS * Rp) == WORDS * Rp
        s.pushDevice([recs.data_ptr()], [WORDS * Rp])
        s.flush()
        nnz = int((vals != 0).sum())
        del vals

        def compact(cap=nnz):
            s.handleFetchCompactRowsDevice(fmt, occ, ptr.data_ptr(), cap and ent[0].data_ptr(), cap and ent[1].data_ptr(),
                                           cap, stream=st.cuda_stream)

        def records():
            s.handleFetchDevice(fmt, occ, recs.data_ptr(), WORDS * Rf, stream=st.cuda_stream)

        def planes():
            s.handleFetchPlanesDevice(fmt, occ, plane[1].data_ptr(), stream=st.cuda_stream)

        def compact_expand():
            compact()
            expand_compact_rows_device(ptr.data_ptr(), ent[0].data_ptr(), ent[1].data_ptr(), WORDS, nnz, COLS,
                                       inv.data_ptr(), WORDS, plane[0].data_ptr(), stream=st.cuda_stream)

        def records_expand():
            records()
            expand_fetch_device(fmt, COLS, recs.data_ptr(), WORDS, inv.data_ptr(), WORDS, plane[0].data_ptr(),
                                stream=st.cuda_stream)

        plane.fill_(-1)
        torch.cuda.synchronize()
        compact_expand(), planes()
        st.synchronize()
        assert int(ptr[-1]) == nnz and torch.equal(plane[0], plane[1]), d
        cands = {k: (lambda f=f: timed(st, f)) for k, f in dict(
            compact=compact, count_only=lambda: compact(0), records=records, planes=planes,
            compact_expand=compact_expand, records_expand=records_expand).items()}
        per_round = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per_round.items()}
        emit(dict(density=d, words=WORDS, cols=COLS, nnz=nnz, record_bytes=WORDS * Rf, compact_bytes=4 * (WORDS + 1) + 8 * nnz,
                  write_pass_ms=round(best["compact"] - best["count_only"], 4),
                  records_over_compact=round(best["records"] / best["compact"], 3),
                  planes_over_compact=round(best["planes"] / best["compact"], 3),
                  records_expand_over_compact_expand=round(best["records_expand"] / best["compact_expand"], 3)),
             per_round, args.out)
        s.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

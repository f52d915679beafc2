#!/usr/bin/env python3
"""Timing of the compact-row batch push against the route it replaces, R successive
handlePushCompactRowsDevice calls. Geometry: config 5's 65 536 words x 1 000 topics split over R owners; each
of the R runs is owner 0's share (words below 65 536 / R, the hot ones under Zipf) of one rank's 2^20 token
moves (per_occ = 2), words uniform or Zipf(1.1), made by Coalescer.run_elems_compact.

One process, candidates alternating (scripts/ubench_coalesce.py's rounds_of): per shape both routes are warmed
up on twin stores, the stores' bytes are compared, then --rounds rounds alternate the two; a round's figure is
the median of --calls calls, HIP events on the caller's stream around the calls and the flush.

  python scripts/ubench_compact_rows_batch.py [--shapes uniform,zipf] [--runs 4,8]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ubench_coalesce import emit, rounds_of, timed  # noqa: E402

WORDS, N, COLS, PER = 65536, 1 << 20, 1000, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="uniform,zipf")
    ap.add_argument("--runs", default="4,8")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_rows_batch_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange
    assert torch.cuda.is_available(), "ubench_compact_rows_batch needs the GPU"
    fmt = DataDesc(1, 1, 0, False, True, False)
    for name in args.shapes.split(","):
        for R in (int(x) for x in args.runs.split(",")):
            own = WORDS // R
            st, co = torch.cuda.Stream(), Coalescer(0)
            co.set_key_range(0, own)
            runs, keep, rows, entries = [], [], 0, 0
            for q in range(R):  # rank q's moves on owner 0's words, as a compact row list
                rng = np.random.default_rng(50 + q)
                keys = (np.minimum(rng.zipf(1.1, size=N), WORDS) - 1 if name == "zipf" else rng.integers(0, WORDS, size=N)).astype(np.int64)
                topics = rng.integers(0, COLS, size=(N, PER)).astype(np.int32)
                sel = keys < own
                keys, topics = keys[sel], topics[sel]
                n, m = len(keys), len(np.unique(keys))
                dk, dc = torch.from_numpy(keys).cuda(), torch.from_numpy(topics).cuda()
                dv = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(n, 1).contiguous()
                ko, po = torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m + 1, dtype=torch.int32, device="cuda")
                eo = torch.empty((2, n * PER), dtype=torch.int32, device="cuda")
                nnz = co.run_elems_compact(fmt, COLS, DeviceKeys(dk.data_ptr(), n), dc.data_ptr(), dv.data_ptr(), PER, ko.data_ptr(),
                                           po.data_ptr(), eo[0].data_ptr(), eo[1].data_ptr(), m, n * PER, stream=st.cuda_stream,
                                           want_entries=True)[1]
                runs.append((DeviceKeys(ko.data_ptr(), m), po.data_ptr(), eo[0].data_ptr(), eo[1].data_ptr()))
                keep.append((ko, po, eo))
                rows, entries = rows + m, entries + nnz
            st.synchronize()

            def store():
                s = DataStore(fmt, KeyRange(0, own - 1), COLS)
                s.fill(float(1 << 30))  # no counter goes negative over the run
                return s

            a, b = store(), store()  # the single calls', the batch's
            distinct = len(np.unique(np.concatenate([k[0].cpu().numpy() for k in keep])))

            def singles():
                for r in runs:
                    a.handlePushCompactRowsDevice(fmt, *r, stream=st.cuda_stream)
                a.flush()

            def batch():
                b.handlePushCompactRowsBatchDevice(fmt, runs, stream=st.cuda_stream)
                b.flush()

            for _ in range(2):
                singles(), batch()
            assert a.values().tobytes() == b.values().tobytes(), (name, R)
            per_round = rounds_of(dict(singles=lambda: timed(st, singles), batch=lambda: timed(st, batch)), args.rounds, args.calls)
            best = {k: min(v) for k, v in per_round.items()}
            emit(dict(shape=name, runs=R, shard_rows=own, cols=COLS, listed_rows=rows, distinct_rows=distinct, entries=entries,
                      singles_over_batch=round(best["singles"] / best["batch"], 3)), per_round, args.out)
            for x in (co, a, b):
                x.close()
            del keep, runs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

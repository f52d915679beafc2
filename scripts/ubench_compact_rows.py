#!/usr/bin/env python3
"""Timing of compact update rows at config 5's geometry: 2^20 token moves (per_occ = 2)
over 65 536 words x 1 000 topics, words uniform or Zipf(1.1). One process, alternating order
(scripts/ubench_coalesce.py's rounds_of):

  source   Coalescer.run_elems_compact against run_elems(records=True) on the same inputs, with both
           outputs' byte counts (the wire sizes) and the measured nnz;
  owner    handlePushCompactRowsDevice + flush against (a) pushDevice of those dense records + flush
           and (b) handlePushElemsDevice on the raw elements + flush.

Per shape every candidate is warmed up, the three owner routes' final shard bytes are compared on triplet
stores, then --rounds rounds alternate the candidates; a round's figure is the median of --calls calls.

  python scripts/ubench_compact_rows.py [--shapes uniform,zipf]
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
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_rows_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, record_bytes
    assert torch.cuda.is_available(), "ubench_compact_rows needs the GPU"
    for name in args.shapes.split(","):
        rng = np.random.default_rng(5)
        topics = rng.integers(0, COLS, size=(N, PER)).astype(np.int32)  # (old, new)
        keys = (np.minimum(rng.zipf(1.1, size=N), WORDS) - 1 if name == "zipf" else rng.integers(0, WORDS, size=N)).astype(np.int64)
        m = len(np.unique(keys))
        fmt = DataDesc(1, 1, 0, False, True, False)
        R = record_bytes(fmt, COLS)[0]

        def store():
            s = DataStore(fmt, KeyRange(0, WORDS - 1), COLS)
            s.fill(float(1 << 30))  # no counter goes negative over the run
            return s

        a, b, e = store(), store(), store()  # the record push's, the compact push's, the element push's
        dk, dc = torch.from_numpy(keys).cuda(), torch.from_numpy(topics).cuda()
        dv = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(N, 1).contiguous()
        recs = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        ko, po = torch.empty(m, dtype=torch.int64, device="cuda"), torch.empty(m + 1, dtype=torch.int32, device="cuda")
        eo = torch.empty((2, N * PER), dtype=torch.int32, device="cuda")
        st, co = torch.cuda.Stream(), Coalescer(0)
        co.set_key_range(0, WORDS)
        occ = DeviceKeys(dk.data_ptr(), N)
        torch.cuda.synchronize()

        def src_compact(want=False):
            return co.run_elems_compact(fmt, COLS, occ, dc.data_ptr(), dv.data_ptr(), PER, ko.data_ptr(), po.data_ptr(),
                                        eo[0].data_ptr(), eo[1].data_ptr(), m, N * PER, stream=st.cuda_stream, want_entries=want)

        def src_records():
            return co.run_elems(fmt, COLS, occ, dc.data_ptr(), dv.data_ptr(), PER, recs.data_ptr(), m * R, records=True,
                                stream=st.cuda_stream)

        def own_records():
            a.pushDevice([recs.data_ptr()], [m * R])
            a.flush()

        def own_compact():
            b.handlePushCompactRowsDevice(fmt, DeviceKeys(ko.data_ptr(), m), po.data_ptr(), eo[0].data_ptr(), eo[1].data_ptr(),
                                          stream=st.cuda_stream)
            b.flush()

        def own_elems():
            e.handlePushElemsDevice(fmt, co, occ, dc.data_ptr(), dv.data_ptr(), PER, stream=st.cuda_stream)
            e.flush()

        nnz = src_compact(True)[1]
        assert tuple(src_records()) == (m, m * R)
        st.synchronize()
        for _ in range(2):  # the same bytes on the three stores
            own_records(), own_compact(), own_elems()
        assert np.array_equal(a.values(), b.values()) and np.array_equal(a.values(), e.values()), name
        cands = dict(src_compact=lambda: timed(st, src_compact), src_records=lambda: timed(st, src_records),
                     own_compact=lambda: timed(st, own_compact), own_records=lambda: timed(st, own_records),
                     own_elems=lambda: timed(st, own_elems))
        per_round = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per_round.items()}
        emit(dict(shape=name, n=N, m=m, cols=COLS, per_occ=PER, nnz=nnz, record_bytes=m * R, compact_bytes=12 * m + 4 + 8 * nnz,
                  src_compact_over_records=round(best["src_compact"] / best["src_records"], 3),
                  own_records_over_compact=round(best["own_records"] / best["own_compact"], 3),
                  own_elems_over_compact=round(best["own_elems"] / best["own_compact"], 3)), per_round, args.out)
        for x in (co, a, b, e):
            x.close()
        del dk, dc, dv, recs, ko, po, eo
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

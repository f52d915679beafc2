#!/usr/bin/env python3
"""Timing of the element push (dml_store_push_elems_device) against, in the same
process, (a) the chain it replaces for a LightLDA worker on the store's GPU: Coalescer.run_elems into
push records (the topic-total array: run_packed of the per-occurrence values), the worker's stream
synchronisation, pushDevice of the records and the flush; and (b) the box's plain copy of
n x 16 + 2 m R bytes (dml_diag_stream, copy = 1), R the row's bytes.

Both routes are timed as scripts/ubench_push_planes.py times them: a HIP event on the caller's stream
in front, the calls as a worker makes them, the store's flush, an event behind. `elems_range` is the
element push with the key range declared. Per shape every candidate is warmed up, the two routes'
final shard bytes are compared on twin stores, then --rounds rounds alternate the candidates; a
round's figure is the median of --calls calls. One JSON line per shape goes to --out.

Shapes, 2^20 token moves (per_occ = 2: -1 on the old topic, +1 on the new) into a 1 M x 1 000 store:
(uniform) 65 536 words; (zipf) Zipf(1.1); (half) one word holding half the list; (c64) uniform into
64 columns; (tot) the 1 000-key topic-total array at 2^21 elements.

  python scripts/ubench_push_elems.py [--shapes uniform,zipf,half,c64,tot]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ubench_coalesce import emit, rounds_of, timed  # noqa: E402

SHAPES = ("uniform", "zipf", "half", "c64", "tot")
WORDS, N = 1 << 20, 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_elems_ubench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from distml_amd import Coalescer, DataDesc, DataStore, DeviceKeys, KeyRange, _lib, record_bytes
    assert torch.cuda.is_available(), "ubench_push_elems needs the GPU"
    L = _lib.load()
    for name in args.shapes.split(","):
        rng = np.random.default_rng(5)
        arr, cols = name == "tot", 1 if name == "tot" else 64 if name == "c64" else 1000
        topics = rng.integers(0, 1000 if arr else cols, size=(N, 2)).astype(np.int32)  # (old, new)
        if arr:
            keys, rows, per = topics.T.reshape(-1).astype(np.int64), 1000, 1
        else:
            keys = (np.minimum(rng.zipf(1.1, size=N), WORDS) - 1 if name == "zipf" else rng.integers(0, 65536, size=N) * 16)
            if name == "half":
                keys[rng.permutation(N)[: N // 2]] = 7
            keys, rows, per = keys.astype(np.int64), WORDS, 2
        n, m = len(keys), len(np.unique(keys))
        fmt = DataDesc(0 if arr else 1, 1, 0, False, True, False)
        R, row = record_bytes(fmt, cols)[0], 4 * cols

        def store():
            s = DataStore(fmt, KeyRange(0, rows - 1), cols)
            s.fill(float(1 << 30))  # no counter goes negative over the run
            return s

        a, b = store(), store()  # the chain's and the element push's
        dk = torch.from_numpy(keys).cuda()
        dc = None if arr else torch.from_numpy(topics).cuda()
        dv = torch.tensor([-1, 1], dtype=torch.int32, device="cuda").repeat(N, 1)
        dv = dv.t().contiguous().view(-1) if arr else dv.contiguous()
        recs = torch.empty(m * R // 4, dtype=torch.int32, device="cuda")
        moved = n * 16 + 2 * m * row
        src = torch.empty(moved, dtype=torch.uint8, device="cuda").fill_(1)
        dst = torch.empty(moved, dtype=torch.uint8, device="cuda")
        st = torch.cuda.Stream()
        co, cor = Coalescer(0), Coalescer(0)
        cor.set_key_range(0, rows)
        torch.cuda.synchronize()

        def chain(c):
            def go():
                if arr:
                    got = c.run_packed(fmt, 1, DeviceKeys(dk.data_ptr(), n), dv.data_ptr(), recs.data_ptr(), m * R, stream=st.cuda_stream)
                else:
                    got = c.run_elems(fmt, cols, DeviceKeys(dk.data_ptr(), n), dc.data_ptr(), dv.data_ptr(), per, recs.data_ptr(),
                                      m * R, records=True, stream=st.cuda_stream)
                assert tuple(got) == (m, m * R)
                st.synchronize()  # a push reads its buffers from the store's own streams
                a.pushDevice([recs.data_ptr()], [m * R])
                a.flush()
            return timed(st, go)

        def elems(c):
            def go():
                b.handlePushElemsDevice(fmt, c, DeviceKeys(dk.data_ptr(), n), dc is not None and dc.data_ptr(), dv.data_ptr(), per,
                                        stream=st.cuda_stream)
                b.flush()
            return timed(st, go)

        def copy():
            ms = C.c_float()
            assert L.dml_diag_stream(1, dst.data_ptr(), src.data_ptr(), moved, C.c_void_p(st.cuda_stream), C.byref(ms)) == 0
            return ms.value

        chain(co), elems(co), chain(cor), elems(cor)  # two calls each: the same bytes on both stores
        assert np.array_equal(a.values(), b.values()), name
        cands = dict(elems=lambda: elems(co), elems_range=lambda: elems(cor), chain=lambda: chain(co),
                     chain_range=lambda: chain(cor), copy=copy)
        per_round = rounds_of(cands, args.rounds, args.calls)
        best = {k: min(v) for k, v in per_round.items()}
        emit(dict(shape=name, n=n, m=m, rows=rows, cols=cols, per_occ=per, row_bytes=row, direct_bytes=moved,
                  copy_gbs=round(2 * moved / best["copy"] / 1e6, 1),
                  elems_over_copy=round(best["elems"] / best["copy"], 3),
                  chain_over_elems=round(best["chain"] / best["elems"], 3),
                  chain_range_over_elems_range=round(best["chain_range"] / best["elems_range"], 3)), per_round, args.out)
        for x in (co, cor, a, b):
            x.close()
        del dk, dc, dv, recs, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

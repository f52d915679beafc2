"""One rank of the native shard group's chained reduce-scatter
(dml_group_push_chained) in a torch-free process, as the PS JVM runs it;
tests/test_native_chain.py starts `world` of these over the RCCL stand-in
(--double, see tests/group_ranks.py) or the system RCCL.

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
import numpy as np

import group_ranks as R

CALLS = 3


def main():
    a, H, uid = R.start()
    from distml_amd import DataDesc
    from distml_amd.group import NativeShardGroup
    import pyoracle
    import chain_expect as X
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
    R.finish(a, H, errors, res)


if __name__ == "__main__":
    main()

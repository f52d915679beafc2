"""One rank of the native shard group's chained reduce-scatter on an AdaGrad
matrix (dml_group_push_chained, FloatMatrixStoreAdaGrad descriptor) in a torch-free
process; tests/test_native_chain_ada.py starts `world` of these over the RCCL
stand-in (--double, see tests/group_ranks.py) or the system RCCL.

Cases (inputs from tests/chain_ada_expect.py, shared with the test's oracle):
  chain   three chained calls back to back, no flush between; call 1: rank 0 passes
          no push; setAlpha on every owner's store after call 0
  order   chained, push_local of the rank's own rows, push_exchange, chained — no
          flush between
  fail    world 3, init with -0.0 rows no push lists: rank 1's call 1 hands over a
          push one byte short; every rank makes every call
  jni     GpuShardGroup's nativeGroupPush mode 4 on the mock JNIEnv with an AdaGrad
          group; data through nativeWriteAll, alpha / delta through nativeSnapshot,
          maxDelta through nativeMaxDelta
Writes out/<case>_<rank>.npz (data, delta, alpha as bytes, md) and prints one JSON line.
"""
import numpy as np

import group_ranks as R


def main():
    a, H, uid = R.start()
    from distml_amd import DataDesc
    from distml_amd.group import NativeShardGroup
    import chain_ada_expect as A
    import chain_expect as X
    world, rank, rows, cols = a.world, a.rank, a.rows, a.cols
    errors, res = [], {}
    first, last = X.shard_ranges(world, rows)[rank]
    fmt = DataDesc(1, 0, 1, False, True, True)

    def put(bufs):
        return [H.put(b) for b in bufs], [b.nbytes for b in bufs]

    def chained(g, c, bufs, lens=None):
        ptrs, ls = put(bufs)
        try:
            g.push_chained(ptrs, lens if lens is not None else ls)
        except Exception as e:
            errors.append([c, type(e).__name__, str(e)[:200]])

    if a.case in ("chain", "order", "fail"):
        g = NativeShardGroup(fmt, rows, cols, rank, world, uid, device=a.device, pieces=a.pieces)
        init = X.minus_zero_init(A.VT, rows, cols) if a.case == "fail" else X.init_values(A.VT, rows, cols)
        g.store.load_values(init[first:last + 1])
        if a.case == "chain":
            calls = A.group_calls(world, rows, cols, bool(a.asc))
            for c in range(A.GROUP_CALLS):
                chained(g, c, calls[c][rank])
                if c == 0:
                    g.store.setAlpha(*A.SET_ALPHA)
        elif a.case == "order":
            calls = A.calls(world, A.GROUP_W, rows, cols, A.GROUP_CALLS, asc=bool(a.asc))
            chained(g, 0, calls[0][rank])
            lp = A.local_push(rank, first, last, cols, world * A.GROUP_W * A.GROUP_CALLS)
            g.push_local(*put([lp]))
            g.push_exchange(*put(calls[1][rank]))
            chained(g, 2, calls[2][rank])
        else:
            calls = A.fail_calls(world, rows, cols)
            for c in range(A.GROUP_CALLS):
                bufs = calls[c][rank]
                lens = [b.nbytes for b in bufs]
                if rank == 1 and c == 1:
                    lens[1] -= 1  # not whole records
                chained(g, c, bufs, lens)
        try:
            g.flush()
        except Exception as e:
            errors.append(["flush", type(e).__name__, str(e)[:200]])
        res["data"] = g.store.values().view(np.uint8)
        alpha, delta = g.store.adagrad_state()
        res["alpha"], res["delta"] = alpha.view(np.uint8), delta.view(np.uint8)
        res["md"] = np.array(g.store.maxDelta(), np.float64)
        g.close()
    elif a.case == "jni":
        from test_jni_shim import MockJVM
        jvm = MockJVM()
        gh, exc = jvm.call("nativeGroupCreate", jvm.bytes_(uid), world, rank, a.device, 1, 0, 1, 0, 1, 1, rows, cols,
                           a.pieces)
        assert exc is None and gh, exc
        st, exc = jvm.call("nativeGroupStore", gh)
        init = X.init_values(A.VT, rows, cols)[first:last + 1]
        jvm.call("nativeReadAll", st, jvm.bytes_(init.view("<u4").astype(">u4").tobytes()))
        calls = A.group_calls(world, rows, cols, bool(a.asc))
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
        n = last - first + 1
        for which, name in ((1, "alpha"), (2, "delta")):
            m = jvm.matrix("F", n, cols)
            _, exc = jvm.call("nativeSnapshot", st, which, 1, 2, m)
            assert exc is None, exc
            res[name] = np.ascontiguousarray(jvm.read_matrix(m, np.float32)).view(np.uint8)
            jvm.L.mock_free(m)
        rc = jvm.prim("I", 2)
        v, exc = jvm.call("nativeMaxDelta", st, rc)
        assert exc is None, exc
        res["md"] = np.array([np.float32(v), *jvm.read_prim(rc, np.int32).tolist()], np.float64)
        jvm.call("nativeGroupDestroy", gh)
    else:
        raise SystemExit(f"unknown case {a.case}")
    R.finish(a, H, errors, res)


if __name__ == "__main__":
    main()

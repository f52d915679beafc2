"""One rank of the native shard group's chained int32 reduce-scatter
(dml_group_push_chained_i32, IntMatrixStore descriptor) in a torch-free process;
tests/test_native_chain_i32.py starts `world` of these over the RCCL stand-in
(--double, see tests/group_ranks.py) or the system RCCL.

Cases (inputs from tests/chain_i32_expect.py, shared with the test's oracle):
  chain   three chained calls back to back, no flush between; call 1: rank 0 passes
          no push
  close   the same, but call 0 closes shard 1 at the rank after its owner
  order   chained (rank 1's own push closes its own shard), push_local of the rank's
          own rows, push_exchange, chained — no flush between
  fail    world 3: rank 2's call 0 hands over a push one byte short, in the call in
          which rank 1's push closes shard 0
  refuse  an fp32 group: dml_group_push_chained_i32 must refuse on every rank
  jni     GpuShardGroup's nativeGroupPush mode 5 on the mock JNIEnv, two clean calls
Every group call and the flush run under one try each: errors lists [where, exception,
key, col]. Writes out/<case>_<rank>.npz (data as bytes) and prints one JSON line.
"""
import numpy as np

import group_ranks as R


def main():
    a, H, uid = R.start(cols=67)
    from distml_amd import DataDesc
    from distml_amd.group import NativeShardGroup
    import chain_expect as X
    import chain_i32_expect as E
    world, rank, rows, cols = a.world, a.rank, a.rows, a.cols
    errors, res = [], {}
    first, last = X.shard_ranges(world, rows)[rank]

    def put(bufs):
        return [H.put(b) for b in bufs], [b.nbytes for b in bufs]

    def attempt(where, fn, *args):
        try:
            fn(*args)
        except Exception as e:
            errors.append([where, type(e).__name__, getattr(e, "key", None), getattr(e, "col", None), str(e)[:160]])

    if a.case in ("chain", "close", "order", "fail"):
        g = NativeShardGroup(DataDesc(1, 0, E.VT), rows, cols, rank, world, uid, device=a.device, pieces=a.pieces)
        g.store.load_values(E.init_counts(rows, cols)[first:last + 1])
        calls = E.group_calls(world, rows, cols, a.case)
        if a.case == "order":
            attempt(0, g.push_chained_i32, *put(calls[0][rank]))
            attempt("local", g.push_local, *put([E.local_push(rank, first, last, cols)]))
            attempt(1, g.push_exchange, *put(calls[1][rank]))
            attempt(2, g.push_chained_i32, *put(calls[2][rank]))
        else:
            for c in range(E.GROUP_CALLS):
                ptrs, lens = put(calls[c][rank])
                if a.case == "fail" and (rank, c) == (2, 0):
                    lens[1] -= 1  # not whole records
                attempt(c, g.push_chained_i32, ptrs, lens)
        attempt("flush", g.flush)
        res["data"] = g.store.values().view(np.uint8)
        res["state"] = np.array(g.store.error_state(), np.int64)
        g.close()
    elif a.case == "refuse":
        g = NativeShardGroup(DataDesc(1, 0, 1), rows, cols, rank, world, uid, device=a.device, pieces=a.pieces)
        init = X.init_values(1, rows, cols)[first:last + 1]
        g.store.load_values(init)
        p = np.zeros(4 + 4 * cols, np.uint8)
        try:
            g.push_chained_i32(*put([p]))
        except Exception as e:
            errors.append([0, type(e).__name__, getattr(e, "code", None), None, str(e)[:160]])
        attempt("flush", g.flush)
        res["data"] = g.store.values().view(np.uint8)
        res["state"] = np.array(g.store.error_state(), np.int64)
        g.close()
    elif a.case == "jni":
        from test_jni_shim import MockJVM
        jvm = MockJVM()
        gh, exc = jvm.call("nativeGroupCreate", jvm.bytes_(uid), world, rank, a.device, 1, 0, 0, 0, 1, 0, rows, cols,
                           a.pieces)
        assert exc is None and gh, exc
        st, exc = jvm.call("nativeGroupStore", gh)
        init = E.init_counts(rows, cols)[first:last + 1]
        jvm.call("nativeReadAll", st, jvm.bytes_(init.view("<u4").astype(">u4").tobytes()))
        calls = E.group_calls(world, rows, cols, "chain")
        for c in range(2):
            bufs = calls[c][rank]
            _, exc = jvm.call("nativeGroupPush", gh, jvm.longs([H.put(b) for b in bufs]),
                              jvm.longs([b.nbytes for b in bufs]), 5)
            if exc:
                errors.append([c, exc[0], None, None, exc[1][:160]])
        _, exc = jvm.call("nativeGroupFlush", gh)
        assert exc is None, exc
        wa, _ = jvm.call("nativeWriteAll", st)
        res["data"] = np.frombuffer(jvm.read(wa), ">u4").astype("<u4").view(np.uint8)
        res["state"] = np.array([0, 0, -1], np.int64)
        jvm.call("nativeGroupDestroy", gh)
    else:
        raise SystemExit(f"unknown case {a.case}")
    R.finish(a, H, errors, res)


if __name__ == "__main__":
    main()

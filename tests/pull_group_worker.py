"""One rank of the native shard group's collective pull (dml_group_pull,
NativeShardGroup.pull) in a torch-free process; tests/test_native_pull.py starts `world`
of these over the RCCL stand-in (--double, see tests/group_ranks.py) or the system RCCL.

Cases (inputs and expected bytes: tests/pull_expect.py):
  table-<store>  one store of the table, the rank's key list pulled in both output orders
                 (AdaGrad: after one push_exchange call, no flush before the pull)
  ord_x / ord_c / ord_ca / ord_i
                 push, pull, pull, push, pull, pull with no flush in between (push_exchange,
                 push_chained fp32 / AdaGrad, push_chained_i32 + push_local); ord_x passes a
                 caller stream and never synchronises between the calls
  closed         chain_i32_expect's "close" call, the flush (the owner's error), then a pull
  cap            the table's f32c67 pull, rank 1's cap one byte short
  jni            GpuShardGroup.pull's native call on the mock JNIEnv
Every output sits 4 bytes past a 16-byte boundary between poisoned guard bands
(geom.OutArena's layout), cap == the expected length exactly. Writes out/<case>_<rank>.npz:
per pull i its bytes b<i>, [rc, out_len] s<i>, counts c<i>, and whether the guards held g<i>.
"""
import ctypes as C

import numpy as np

import group_ranks as R


def main():
    a, H, uid = R.start()
    from distml_amd import DataDesc, _lib
    from distml_amd.group import NativeShardGroup
    import chain_i32_expect as E
    import geom
    import pull_expect as P
    world, rank = a.world, a.rank
    errors, res, outs = [], {}, []
    L = _lib.load()
    H.h.hipMemcpy.restype = C.c_int

    class Out:
        """geom.OutArena on this process's HIP runtime."""

        def __init__(self, nbytes):
            self.a = geom.OutArena(nbytes, 4)
            self.base = H.put(self.a.host)
            assert self.base % 256 == 0
            self.ptr = self.base + self.a.off

        def read(self, written):
            back = np.empty_like(self.a.host)
            assert H.h.hipMemcpy(back.ctypes.data, self.base, back.nbytes, 2) == 0  # device to host
            self.a.back = back
            try:
                self.a.untouched([(0, written)])
                held = True
            except AssertionError as e:
                errors.append(["guard", str(e)[:200]])
                held = False
            return back[self.a.off:self.a.off + self.a.nbytes].copy(), held

    def setup(tag, init):
        dt, kt, vt, ada, rows, cols = P.SPECS[tag]
        g = NativeShardGroup(DataDesc(dt, kt, vt, False, True, ada), rows, cols, rank, world, uid, device=a.device,
                             pieces=a.pieces)
        if ada:
            g.store.setAlpha(*P.ADA)
        p = P.parts(tag, world)[rank]
        g.store.load_values(init[p.firstKey:p.lastKey + 1])
        return g

    def put(bufs):
        return [H.put(b) for b in bufs], [b.nbytes for b in bufs]

    def prepare(tag, keys):
        """A pull's device buffers, made before the call: (keys, output arena, bytes expected)."""
        need = sum(len(q) for q in P.split(tag, world, keys)) * P.record_bytes(tag)
        return H.put(keys if len(keys) else np.zeros(1, np.int64)), Out(need), need

    def pull(g, prepared, nkeys, request_order, stream=0, short=0, bound=False):
        """Enqueue one pull; the bytes are read in collect()."""
        dk, o, need = prepared
        if bound:  # through the Python binding
            ln, counts = g.pull(dk, nkeys, o.ptr, need, request_order, stream)
            rc = 0
        else:
            ln, cn = C.c_int64(-7), (C.c_int64 * world)()
            rc = L.dml_group_pull(C.c_void_p(g._h), C.c_void_p(dk), nkeys, C.c_void_p(o.ptr), need - short,
                                  _lib.DML_PULL_REQUEST_ORDER if request_order else 0, C.byref(ln), cn,
                                  C.c_void_p(stream or None))
            ln, counts = ln.value, list(cn)
        outs.append((o, rc, ln, counts, 0 if rc else ln))

    def collect():
        for i, (o, rc, ln, counts, written) in enumerate(outs):
            b, held = o.read(written)
            res[f"b{i}"], res[f"s{i}"], res[f"c{i}"], res[f"g{i}"] = b, np.array([rc, ln]), np.array(counts), np.array(held)

    def attempt(where, fn, *args):
        try:
            fn(*args)
        except Exception as e:
            errors.append([where, type(e).__name__, getattr(e, "key", None), getattr(e, "col", None), str(e)[:160]])

    case = a.case
    if case.startswith("table-") or case == "cap":
        tag = "f32c67" if case == "cap" else case[len("table-"):]
        g = setup(tag, P.init_values(tag))
        keys = P.key_lists(tag, world)[rank]
        if tag == "ada":
            g.push_exchange(*put(P.ada_first_call(world)[rank]))
        short = 1 if case == "cap" and rank == 1 else 0
        pull(g, prepare(tag, keys), len(keys), False, short=short, bound=case != "cap")
        pull(g, prepare(tag, keys), len(keys), True, short=short)
        attempt("flush", g.flush)
        collect()
        g.close()
    elif case in P.ORDER:
        tag, _, path = P.ORDER[case]
        g = setup(tag, P.order_init(tag))
        keys = P.key_lists(tag, world)[rank]
        stream = 0
        if case == "ord_x":  # a non-blocking stream: no copy on the null stream orders it
            s = C.c_void_p()
            assert H.h.hipStreamCreateWithFlags(C.byref(s), 1) == 0
            stream = s.value
        push = {"exchange": g.push_exchange, "chained": g.push_chained, "chained_i32": g.push_chained_i32}[path]
        # every buffer is on the device before the first call: nothing below copies or waits
        bufs = [put(P.pushes(tag, rank, c)) for c in range(2)]
        local = [put([P.local_push(tag, rank, world)]) for c in range(2)]
        prepared = [prepare(tag, keys) for _ in range(4)]
        for c in range(2):
            attempt(c, push, *bufs[c])
            if path == "chained_i32":
                attempt(f"local{c}", g.push_local, *local[c])
            pull(g, prepared[2 * c], len(keys), False, stream)
            pull(g, prepared[2 * c + 1], len(keys), True, stream)
        if stream:
            H.h.hipStreamSynchronize.argtypes = [C.c_void_p]
            assert H.h.hipStreamSynchronize(C.c_void_p(stream)) == 0
        collect()
        attempt("flush", g.flush)
        g.close()
    elif case == "closed":
        tag = P.CLOSED[0]
        rows, cols = P.SPECS[tag][4], P.SPECS[tag][5]
        g = setup(tag, E.init_counts(rows, cols))
        attempt(0, g.push_chained_i32, *put(E.group_calls(world, rows, cols, "close")[0][rank]))
        attempt("flush", g.flush)
        keys = P.key_lists(tag, world)[rank]
        pull(g, prepare(tag, keys), len(keys), False)
        pull(g, prepare(tag, keys), len(keys), True)
        collect()
        res["state"] = np.array(g.store.error_state(), np.int64)
        g.close()
    elif case == "jni":
        from test_jni_shim import MockJVM
        tag = "f32c67"
        dt, kt, vt, ada, rows, cols = P.SPECS[tag]
        jvm = MockJVM()
        f = getattr(jvm.L, "Java_com_intel_distml_util_store_GpuShardGroup_nativeGroupPull")
        f.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int64] * 5 + [C.c_int32] * 2
        f.restype = C.c_void_p
        jvm.fn["nativeGroupPull"] = f
        gh, exc = jvm.call("nativeGroupCreate", jvm.bytes_(uid), world, rank, a.device, dt, kt, vt, 0, 1, int(ada), rows,
                           cols, a.pieces)
        assert exc is None and gh, exc
        st, exc = jvm.call("nativeGroupStore", gh)
        p = P.parts(tag, world)[rank]
        init = P.init_values(tag)[p.firstKey:p.lastKey + 1]
        jvm.call("nativeReadAll", st, jvm.bytes_(init.view("<u4").astype(">u4").tobytes()))
        keys = P.key_lists(tag, world)[rank]
        for flags in (0, 1):
            dk, o, need = prepare(tag, keys)
            arr, exc = jvm.call("nativeGroupPull", gh, dk, len(keys), o.ptr, need, flags, world)
            assert exc is None, exc
            counts = np.frombuffer(jvm.read(arr), "<i8")
            outs.append((o, 0, int(counts.sum()) * P.record_bytes(tag), counts.tolist(), need))
        collect()
        _, exc = jvm.call("nativeGroupFlush", gh)
        assert exc is None, exc
        jvm.call("nativeGroupDestroy", gh)
    else:
        raise SystemExit(f"unknown case {case}")
    R.finish(a, H, errors, res)


if __name__ == "__main__":
    main()

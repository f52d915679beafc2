"""One store driven through a mixed life, against the CPU oracle after every burst.

tests/opseq.py makes the sequences (bursts of pipelined device push calls of every kind
the store dispatches on, planned errors, a read / checkpoint / reset op behind each
burst); tests/test_opseq.py checks their plan on the oracle alone. Here a
`DataStore(..., async_push=True)` and an `OracleStore` take the same ops side by side.
Every comparison is of bits (unsigned views: -0.0 is not +0.0, NaN payloads count).
A failure names the op that broke; at the end the counters and kernel names must show
the paths the sequence planned (counted from the plan, not from the store).
"""
import ctypes as C
import io
import json

import numpy as np
import pytest

import opseq
import sparse_route

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.init()


def _bits(a, vt):
    return np.ascontiguousarray(a).view(opseq.UDT[vt])


class _Runner:
    def __init__(self, oracle, cfg, seq):
        from distml_amd import DataDesc, DataStore, KeyRange
        self.cfg, self.seq = cfg, seq
        self.fmt = DataDesc(cfg["data_type"], cfg["key_type"], cfg["value_type"], False, True, cfg["ada"])
        self.s = DataStore(self.fmt, KeyRange(cfg["first"], cfg["first"] + cfg["rows"] - 1), cfg["cols"],
                           float_array_ref_stride=cfg["ref_stride"], async_push=True)
        self.side = opseq.OracleSide(oracle, cfg, seq[0])
        self.s.load_values(seq[0]["values"])
        if cfg["ada"]:
            self.s.setAlpha(*seq[0]["alpha"])
            if opseq.flat_shaped(cfg):
                self.s.set_knob(1, 0)  # DML_KNOB_IDENT_FULL_MIN_BYTES: k_ada_ident at this size
        self.names = set()
        self.route_lo, self.route_hi = {}, {}  # the sparse counters the calls' bytes plan (arrays)
        self.at = 0     # index of the op being applied
        self.op = None

    def note_kernel(self):
        n = self.s.kernel_name()
        if n:
            self.names.add(n.split("<")[0].replace("dml::", ""))

    def where(self):
        calls = [o["kind"] for o in self.burst]
        return (f"{self.cfg['name']}: op {self.at} ({self.op['op']} {self.op['kind']}), burst {calls}, "
                f"last kernel {self.s.kernel_name()!r}, stats {self.s.stats()}")

    def same(self, what, got, want):
        if isinstance(want, bytes):
            if got != want:
                g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
                n = min(len(g), len(w))
                at = np.nonzero(g[:n] != w[:n])[0]
                pytest.fail(f"{what}: {len(got)} bytes against {len(want)}, first difference at byte "
                            f"{at[:1].tolist()}, {len(at)} bytes differ; {self.where()}")
            return
        vt = opseq.F32 if want.dtype == np.float32 else self.cfg["value_type"]
        g, w = _bits(got, vt), _bits(want, vt)
        assert g.shape == w.shape, (what, g.shape, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).any(axis=1))[0]
            r = int(rows[0])
            c = np.nonzero(g[r] != w[r])[0]
            pytest.fail(f"{what}: {len(rows)} rows differ, first rows {rows[:8].tolist()}; row {r} cols "
                        f"{c[:6].tolist()} got {np.asarray(got)[r, c[:6]]} want {np.asarray(want)[r, c[:6]]}; "
                        f"{self.where()}")

    def compare_state(self):
        s, o = self.s, self.side.o
        self.same("values()", s.values(), o.data)
        if self.cfg["ada"]:
            a, d = s.adagrad_state()
            self.same("alpha", a, o.alpha)
            self.same("delta", d, o.delta)
            assert s.maxDelta() == o.max_delta(), ("maxDelta", s.maxDelta(), o.max_delta(), self.where())

    def store_sync(self, op):
        """The store's call of a sync op: what it returns (bytes / rows), or None."""
        from distml_amd import KeyList, KeyRange, _lib
        from distml_amd.store import check
        s, kind = self.s, op["kind"]
        if kind == "flush":
            s.flush()
        elif kind == "fetch_list":
            return s.handleFetch(self.fmt, KeyList(op["keys"]))
        elif kind == "fetch_range":
            return s.handleFetch(self.fmt, KeyRange(op["lo"], op["hi"]))
        elif kind == "write_all":
            return s.writeAll()
        elif kind == "sync_to":
            buf = io.BytesIO()
            s.syncTo(buf, op["lo"], op["hi"])
            return buf.getvalue()
        elif kind == "sync_from":
            s.syncFrom(io.BytesIO(op["data"]), op["lo"], op["hi"])
        elif kind == "read_all":
            s.readAll(io.BytesIO(op["data"]))
        elif kind == "fill":
            if op["as_set"]:
                s.set(repr(float(op["value"])))
            else:
                s.fill(op["value"])
        elif kind == "set_alpha":
            s.setAlpha(*op["alpha"])
        elif kind == "read_rows":
            n = op["hi"] - op["lo"] + 1
            out = np.empty((n, self.cfg["cols"]), s.dtype if op["which"] == 0 else np.float32)
            check(_lib.load().dml_store_read_rows(s._h, op["which"], op["lo"], n, out.ctypes.data, out.nbytes), s)
            return out
        return None

    def plan_route(self, call, failed):
        """Array stores: the sparse counters tests/sparse_route.py derives from the call's bytes. A
        call the oracle applied whole counts exactly; the call that fails counts as an upper bound
        (its chunks behind the failing one are dropped, and the model does not see which chunk an
        int32 negative counter is in)."""
        cfg = self.cfg
        if cfg["data_type"] != opseq.ARRAY:
            return
        routes = sparse_route.call_routes(cfg["value_type"], cfg["key_type"], cfg["first"], cfg["rows"],
                                          [bytes(p) for p in call["pushes"]], 8 if cfg["ref_stride"] else None)
        if not routes:
            return
        for k, v in sparse_route.expect(routes)[0].items():
            self.route_hi[k] = self.route_hi.get(k, 0) + v
            if not failed:
                self.route_lo[k] = self.route_lo.get(k, 0) + v

    def took(self, e, want_err, raised):
        """A store exception is legal only once the oracle has failed in this burst; anything
        that is not one of the reference's three push errors (a HIP error, say) goes up as it is."""
        if e.code not in (opseq.E_KEY, opseq.E_TRUNC, opseq.E_NEG):
            raise e
        assert want_err is not None, f"unplanned {type(e).__name__} {(e.code, e.key, e.col)}: {self.where()}"
        raised.append(e)

    def run(self):
        from distml_amd import DistMLException
        s, side = self.s, self.side
        at = 1
        for bi, (calls, sync) in enumerate(opseq.bursts_of(self.seq)):
            self.burst = calls
            want_err, raised, keep = None, [], []
            for call in calls:
                self.at, self.op = at, call
                at += 1
                if want_err is None:
                    assert call["applied"]
                    want_err = side.push_call(call)
                    self.plan_route(call, failed=want_err is not None)
                dev = [torch.from_numpy(p).cuda() for p in call["pushes"]]
                keep.append(dev)  # alive to the end of the burst
                torch.cuda.synchronize()
                try:
                    s.pushDevice([d.data_ptr() for d in dev], [d.numel() for d in dev])
                except DistMLException as e:
                    self.took(e, want_err, raised)
                self.note_kernel()
            self.at, self.op = at, sync
            at += 1
            got, redo = None, False
            try:
                if sync["end"] == "retire":
                    s.retire(s.push_seq())
            except DistMLException as e:
                self.took(e, want_err, raised)
            try:
                got = self.store_sync(sync)
            except DistMLException as e:
                self.took(e, want_err, raised)
                redo = True
            if want_err is not None:
                assert raised, f"the oracle failed with {want_err}, the store raised nothing: {self.where()}"
                e = raised[0]
                assert (e.code, e.key, e.col) == tuple(want_err), ((e.code, e.key, e.col), want_err, self.where())
                for e in raised[1:]:  # the failed-state refusal
                    assert e.code == want_err[0], ((e.code, e.key, e.col), want_err, self.where())
                assert s.error_state() == tuple(want_err), (s.error_state(), want_err, self.where())
                s.clear_error()
                side.clear_error()
                if redo:
                    got = self.store_sync(sync)
            else:
                assert not raised
            want = side.sync(sync)
            if want is not None:
                self.same(sync["kind"], got, want)
            self.compare_state()
            self.note_kernel()
            del keep
        return s.stats()

    def close(self):
        self.s.close()
        self.side.o.close()


@pytest.mark.parametrize("name,seed", opseq.CASES)
def test_sequence_matches_oracle(oracle, name, seed):
    cfg = opseq.CONFIGS[name]
    seq = opseq.make_sequence(name, seed)
    r = _Runner(oracle, cfg, seq)
    try:
        st = r.run()
        planned = opseq.expected_paths(seq)
        print("OPSEQ " + json.dumps(dict(config=name, seed=seed, kernels=sorted(r.names), planned=planned,
                                         stats={k: v for k, v in st.items() if v})))
        # a sequence that stopped reaching a path fails: each applied call that plans one counts
        reached = {"spec": st["spec_chunks"], "rerun": st["spec_reruns"], "reuse": st["reused_pushes"],
                   "identity": st["identity_pushes"], "ident_launch": st["ident_launches"],
                   "sparse_skew": st["sparse_replays"] + st["sparse_big_chunks"],
                   "k_ada_ident": int("k_ada_ident" in r.names), "k_ada_flat": int("k_ada_flat" in r.names)}
        for path, n in planned.items():
            need = 1 if path.startswith("k_") or path == "sparse_skew" else n
            assert reached[path] >= need, (path, reached[path], need, st, sorted(r.names))
        if not opseq.spec_shaped(cfg):
            assert st["spec_chunks"] == 0, st
        # array stores: every applied call took the route the model derives from its bytes
        for k, hi in r.route_hi.items():
            assert r.route_lo.get(k, 0) <= st[k] <= hi, (k, r.route_lo.get(k, 0), st[k], hi)
    finally:
        r.close()


def test_fetch_refuses_keys_outside_the_range(oracle):
    """dml_store_fetch checks keys by range, not by indexOf's narrowed (int)(key - first): a
    64-bit key congruent to an in-shard key modulo 2^32 is refused before any copy or launch
    (the reference intersects a fetch's keys with the shard first), with the error state and
    out_len as documented; after clear_error the store fetches as before."""
    from distml_amd import DataDesc, DataStore, KeyList, KeyRange, _lib, encode_matrix_push
    from distml_amd._lib import DML_E_KEY_OUT_OF_SHARD
    first, rows, cols = (1 << 34) + 500, 100, 5
    last = first + rows - 1
    fmt = DataDesc(1, 1, 1)
    s = DataStore(fmt, KeyRange(first, last), cols, async_push=True)
    o = oracle.OracleStore(1, 1, 1, first, last, cols)
    rng = np.random.default_rng(8)
    init = rng.standard_normal((rows, cols)).astype(np.float32)
    s.load_values(init)
    o.data[:] = init
    push = encode_matrix_push(first + rng.permutation(rows), rng.standard_normal((rows, cols)), 1, 1)
    s.handlePush(fmt, push)
    assert o.push(push) == 0
    L = _lib.load()
    rec = 8 + 4 * cols
    for bad in (first + (1 << 32) + 3, first - (1 << 32) + 3, last + 1):
        keys = (C.c_int64 * 3)(first + 1, bad, first + 2)
        out = np.zeros(3 * rec, np.uint8)
        out_len = C.c_int64(-1)
        rc = L.dml_store_fetch(s._h, keys, 3, out.ctypes.data, out.nbytes, C.byref(out_len))
        assert rc == DML_E_KEY_OUT_OF_SHARD
        assert s.error_state() == (DML_E_KEY_OUT_OF_SHARD, bad, -1)
        assert out_len.value == 3 * rec
        assert not out.any()  # nothing was copied
        s.clear_error()
        want = [last, first, first + 3, first + 50]
        assert s.handleFetch(fmt, KeyList(want)) == o.fetch(want)
    assert s.values().tobytes() == o.data.tobytes()
    s.close()

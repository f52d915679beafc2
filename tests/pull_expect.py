"""The yardstick of the collective group pull (dml_group_pull), and the inputs of its GPU
tests (tests/pull_group_worker.py, tests/test_native_pull.py), so that
tests/test_pull_expect.py can pin both on the CPU.

Shard s of KeyRange(0, rows-1).linearSplit(world) is one reference store (the CPU oracle)
over that shard's key range. A Model is fed the group's calls in the documented order of
each push path — push_exchange rank-major, push_chained / push_chained_i32 in ring order
(rank s, s+1, ..., s-1), push_local the owner's own push — each push restricted to the shard's
records; an int32 shard whose push leaves a counter negative takes nothing more. A pull is
WorkerAgent.fetch (WorkerAgent.java:74-122): the rank's keys intersected with every
partition in list order (KeyRange.intersect of a KeyList, without KeyList's de-duplication:
a key listed twice gets two records), one oracle fetch per owner; the answers concatenated
owner-major, or laid out in request order (record j = the j-th key inside the model).
"""
import numpy as np

import chain_expect as X
import chain_i32_expect as E  # noqa: F401  (registers the int32 entry of chain_expect's dtype tables)
import fetch_cases as fc

ADA = fc.ADA
# tag -> (data type, key type, value type, AdaGrad, rows, cols)
SPECS = {
    "f32c67": (1, 0, 1, False, 1000, 67),      # shards 334 / 334 / 332 at world 3
    "f32c256": (1, 0, 1, False, 1000, 256),
    "f32c768k8": (1, 1, 1, False, 200, 768),   # long keys; 770 dwords: the 16-byte-load side of kFetchVloadMinDw
    "ada": (1, 0, 1, True, 1000, 200),         # after a push that moves alpha
    "i32": (1, 0, 0, False, 1000, 67),
    "f64": (1, 0, 3, False, 1000, 3),
    "af32": (0, 0, 1, False, 1000, 1),         # FloatArrayStore: 8-byte slot, zero pad
    "ai32": (0, 0, 0, False, 1000, 1),
    "af64": (0, 0, 3, False, 1000, 1),
}
# the world every store of the table runs at (world 1 runs f32c67 on the system RCCL)
TABLE = [("f32c67", 3), ("f32c256", 2), ("f32c768k8", 4), ("ada", 3), ("i32", 2), ("f64", 4), ("af32", 3),
         ("ai32", 2), ("af64", 4), ("f32c67", 1)]


def case_of(tag):
    dt, kt, vt, ada, rows, cols = SPECS[tag]
    return fc._case(tag, dt, kt, vt, cols, rows, 0, ada)


def record_bytes(tag):
    return fc.record_bytes(case_of(tag))


def init_values(tag):
    """rows x cols with fetch_cases' specials (-0.0, denormals, Inf, NaN payloads; INT_MIN / INT_MAX);
    int32 matrices that take pushes start from chain_i32_expect's counts instead."""
    return fc.build_init(case_of(tag))


def parts(tag, world):
    from distml_amd.datadesc import KeyRange
    return KeyRange(0, SPECS[tag][4] - 1).linearSplit(world)


# ---- key lists, one kind per rank -----------------------------------------------------------
KINDS = {1: ["edges"], 2: ["desc700", "empty"], 3: ["edges", "own257", "remote1"],
         4: ["empty", "desc700", "remote257", "edges"]}


def key_list(kind, tag, world, rank):
    rows = SPECS[tag][4]
    ps = parts(tag, world)
    rng = np.random.default_rng(1000 * world + rank)
    if kind == "edges":
        # every shard's first and last key, last shard first; the keys outside the model between
        # them; two keys listed twice
        k = []
        for p in reversed(ps):
            k += [p.lastKey, -1, p.firstKey, rows, 1 << 40]
        k += [ps[0].firstKey, ps[-1].lastKey, -(1 << 33), (1 << 32) + 5]
        return np.array(k, np.int64)
    if kind == "desc700":  # descending, the last 57 a repeat of the first
        n = min(rows, 643)
        k = np.arange(rows - 1, rows - 1 - n, -1)
        return np.concatenate([k, k[:700 - n]]).astype(np.int64) if rows >= 643 else \
            np.resize(k, 700).astype(np.int64)
    if kind == "own257":   # only the rank's own shard
        p = ps[rank]
        return rng.integers(p.firstKey, p.lastKey + 1, size=257).astype(np.int64)
    if kind == "remote257":  # only one remote shard
        p = ps[(rank + 1) % world]
        return rng.integers(p.firstKey, p.lastKey + 1, size=257).astype(np.int64)
    if kind == "remote1":  # one key of one remote shard
        return np.array([ps[(rank + 1) % world].lastKey], np.int64)
    assert kind == "empty"
    return np.zeros(0, np.int64)


def kinds(world):
    """The kind of every rank's list (worlds past 4, the all-devices run: the six kinds in turn)."""
    every = ("edges", "own257", "remote1", "desc700", "empty", "remote257")
    return KINDS.get(world) or [every[r % len(every)] for r in range(world)]


def key_lists(tag, world):
    return [key_list(k, tag, world, r) for r, k in enumerate(kinds(world))]


def split(tag, world, keys):
    """Per owner, the keys of `keys` inside its partition in list order: KeyCollection.intersect's
    loop (`k for k in keys if self.contains(k)`) over the list itself."""
    return [[int(k) for k in keys if p.contains(int(k))] for p in parts(tag, world)]


# ---- pushes -----------------------------------------------------------------------------------
def pushes(tag, rank, call, W=2, even=False):
    """W pushes of one rank and call: a seeded half of the rows (even: of the even rows) in a
    seeded order (int keys)."""
    from distml_amd.store import encode_matrix_push
    dt, kt, vt, ada, rows, cols = SPECS[tag]
    assert dt == 1 and kt == 0
    out = []
    for b in range(W):
        r = np.random.default_rng(7000 + 100 * call + 10 * rank + b)
        keys = r.permutation(np.arange(0, rows, 2 if even else 1))[: rows // 2]
        if vt == 0:
            vals = r.integers(0, 4, size=(len(keys), cols)).astype(np.int32)
        else:
            vals = (r.standard_normal((len(keys), cols)) * (0.6 if ada else 0.1)).astype(X.VDT[vt])
        out.append(np.frombuffer(encode_matrix_push(keys, vals, kt, vt), np.uint8).copy())
    return out


def local_push(tag, rank, world):
    """One push of the rank's own rows, descending keys, int32 counts."""
    from distml_amd.store import encode_matrix_push
    p = parts(tag, world)[rank]
    keys = np.arange(p.firstKey, p.lastKey + 1)[::-1]
    vals = np.random.default_rng(7700 + rank).integers(0, 4, size=(len(keys), SPECS[tag][5])).astype(np.int32)
    return np.frombuffer(encode_matrix_push(keys, vals, 0, 0), np.uint8).copy()


class Model:
    """One oracle store per shard, fed in the documented order of each push path."""

    def __init__(self, oracle, tag, world, init=None):
        dt, kt, vt, ada, rows, cols = SPECS[tag]
        self.tag, self.world, self.vt, self.cols = tag, world, vt, cols
        self.parts = parts(tag, world)
        init = init_values(tag) if init is None else init
        self.stores, self.closed = [], [False] * world
        for p in self.parts:
            o = oracle.OracleStore(dt, kt, vt, p.firstKey, p.lastKey, cols, 1, int(ada))
            if ada:
                o.set_alpha(*ADA)
            o.data[:] = init[p.firstKey:p.lastKey + 1]
            self.stores.append(o)

    def close(self):
        for o in self.stores:
            o.close()

    def _feed(self, s, push, restrict=True):
        p = self.parts[s]
        b = X.restrict(push, self.vt, self.cols, p.firstKey, p.lastKey) if restrict else bytes(push)
        if b and not self.closed[s]:
            self.closed[s] = self.stores[s].push(b) != 0

    def exchange(self, per_rank):
        for s in range(self.world):
            for r in X.rank_major(self.world, s):
                for p in per_rank[r]:
                    self._feed(s, p)

    def chained(self, per_rank):
        for s in range(self.world):
            for r in X.rotated(self.world, s):
                for p in per_rank[r]:
                    self._feed(s, p)

    def local(self, per_rank_push):
        for s in range(self.world):
            self._feed(s, per_rank_push[s], restrict=False)

    def pull(self, keys):
        """(owner-major bytes, request-order bytes, counts) of one rank's list."""
        per = split(self.tag, self.world, keys)
        om = b"".join(self.stores[q].fetch(np.array(per[q], np.int64)) for q in range(self.world))
        counts = [len(k) for k in per]
        rec = record_bytes(self.tag)
        recs = np.frombuffer(om, np.uint8).reshape(-1, rec)
        kept = [int(k) for k in keys if any(p.contains(int(k)) for p in self.parts)]
        owner = np.array([next(q for q, p in enumerate(self.parts) if p.contains(k)) for k in kept], np.int64)
        req = np.empty_like(recs)
        req[np.argsort(owner, kind="stable")] = recs  # owner-major record i is kept key order[i]'s
        return om, req.tobytes(), counts

    def pulls(self, lists):
        return [self.pull(k) for k in lists]


# ---- the cases of tests/test_native_pull.py beyond the table --------------------------------
def ada_first_call(world):
    """The AdaGrad table case's one push_exchange call (it moves alpha off its initial value):
    even rows only, as in fetch_cases, so that no special of the odd rows meets arithmetic."""
    return [pushes("ada", r, 0, W=1, even=True) for r in range(world)]


ORDER = {  # case -> (store, world, push path); every case: push, pull, push, pull, no flush
    "ord_x": ("f32c67", 3, "exchange"),
    "ord_c": ("f32c67", 3, "chained"),
    "ord_ca": ("ada", 2, "chained"),
    "ord_i": ("i32", 3, "chained_i32"),  # each chained call followed by a push_local
}


def order_init(tag):
    """The ordering cases add to every row: counts no push drives negative, or values without specials."""
    if SPECS[tag][2] == 0:
        return E.init_counts(SPECS[tag][4], SPECS[tag][5])
    return fc.build_init(case_of(tag), plain=True)


def order_expected(oracle, case):
    """[pull 0's, pull 1's] lists of per-rank (owner-major, request-order, counts)."""
    tag, world, path = ORDER[case]
    m = Model(oracle, tag, world, order_init(tag))
    lists = key_lists(tag, world)
    out = []
    for c in range(2):
        per_rank = [pushes(tag, r, c) for r in range(world)]
        if path == "exchange":
            m.exchange(per_rank)
        else:
            m.chained(per_rank)
        if path == "chained_i32":
            m.local([local_push(tag, r, world) for r in range(world)])
        out.append(m.pulls(lists))
    m.close()
    return out


CLOSED = ("i32", 3)


def closed_expected(oracle):
    """chain_i32_expect's "close" inputs, call 0: shard 1 closes; the pull after the flush."""
    tag, world = CLOSED
    rows, cols = SPECS[tag][4], SPECS[tag][5]
    m = Model(oracle, tag, world, E.init_counts(rows, cols))
    m.chained(E.group_calls(world, rows, cols, "close")[0])
    assert m.closed == [False, True, False]
    out = m.pulls(key_lists(tag, world))
    m.close()
    return out


def table_expected(oracle, tag, world):
    m = Model(oracle, tag, world)
    if tag == "ada":
        m.exchange(ada_first_call(world))
    out = m.pulls(key_lists(tag, world))
    m.close()
    return out

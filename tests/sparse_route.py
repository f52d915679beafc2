"""The route an array chunk takes through dml_sparse.hip, restated in integer Python and numpy
from the C++ (line numbers: distml_amd/csrc/dml_sparse.hip unless a file is named), never from
what a kernel or a counter reports. tests/test_sparse_route.py checks `plan` against the
library's own dml_diag_sparse_plan over a sweep and checks that every case of
tests/sparse_cases.py is on the route it claims; tests/test_gpu_sparse_edges.py then asserts
the counters and the kernel name `route` predicts.

plan    sparse_plan (1015-1038), plan_leaves (1000-1013), sparse_compact_ok (1081-1083),
        sparse_plan_big (1046-1079), sparse_leaf_bshift / sparse_big_bshift (1085-1095), in
        launch_chunk's order (dml_store.hip:249-253).
route   what the kernels count against those capacities, from a chunk's actual keys:
          k_sp_l1_fast (629-633)   records of a level-1 bin (row >> SL >> D2) > cap1
          k_sp_l2_fast (695-698)   records of a leaf (row >> SL) > cap2
          k_sp_l1_big  (815-816)   records of a (big leaf row >> BL, slice push % 8) > capS
        any of them sets SpStat::overflow, and launch_chunk (dml_store.hip:279-292) then runs
        the counted partition, as it does when compact records meet a cutoff. Every record whose
        key lies in the shard is counted, also those at or past the cutoff (they keep their slot
        and are never applied). The leaf kernels flag a leaf they do not apply:
          k_sp_leaf (404-410), k_sp_leaf_big (868-874)   more than kSpLeafCap / kSpBigCap records
          k_sp_leaf (488-491), k_sp_leaf_big (953)       an applied record's line bucket
                                                         (row - leaf's first row) >> bshift holds
                                                         more than kSpBucketMax records (all of
                                                         the bucket's records count, applied or not)
          k_sp_leaf (500-502), k_sp_leaf_big (962)       compact words: one push lists a row twice
        and a flagged leaf sends the chunk to sparse_replay (1341-1426), whose four branches are
        numbered as DESIGN.md §4.5 does: 1 big (re-plan with BL, re-partition counted), 2 compact
        (re-partition counted), 3 single-pass full records (k_sp_pack_flagged, sort, k_sp_runs),
        4 counted (hm.kept, sort, k_sp_runs).
"""
import numpy as np

K_MAX_W = 64             # kMaxW (dml_internal.h:15): pushes per chunk
K_TILE = 4096            # kSpTile (dml_internal.h:279)
K_LEAF_CAP = 2048        # kSpLeafCap
K_BIG_CAP = 4096         # kSpBigCap
K_BIG_BINS = 16384       # kSpBigBins
K_SLICES = 8             # kSpSlices
K_COMPACT_ROW_BITS = 26  # kSpCompactRowBits (dml_internal.h:310)
K_LEAF_THREADS = 512     # kSpLeafThreads (318), kSpBigThreads (844)
K_LINES = 2 * K_LEAF_THREADS  # kSpLines (323), kSpBigLines (845)
K_BUCKET_MAX = 64        # kSpBucketMax (324)
I32, F32, F64 = 0, 1, 3  # VType (dml_internal.h:197) = DML_ELEMENT_TYPE_*

FIELDS = ("nrec", "nleaves", "SL", "D2", "nbins1", "cap1", "cap2", "compact", "big", "BL", "nbig", "capS",
          "bshift")


def ceil_log2(x):
    """993-997."""
    r = 0
    while (1 << r) < x:
        r += 1
    return r


def _cdiv_pow2(x, sh):
    return (x + (1 << sh) - 1) >> sh


def plan_leaves(nrec, rows, SL):
    """1000-1013: the SL-dependent fields."""
    nleaves = _cdiv_pow2(rows, SL)                                   # 1002
    D2 = min(8, ceil_log2(nleaves))                                  # 1003
    nbins1 = _cdiv_pow2(nleaves, D2)                                 # 1004
    cap1 = (nrec // max(nbins1, 1)) * 2 + K_TILE                     # 1010
    cap2 = min(K_LEAF_CAP, 2 * (nrec // max(nleaves, 1)) + 256)      # 1011
    return dict(SL=SL, nleaves=nleaves, D2=D2, nbins1=nbins1, cap1=cap1, cap2=cap2)


def leaf_bshift(SL, lines=K_LINES):
    """1085-1095: the smallest shift that fits 2^SL rows into `lines` buckets."""
    b = 0
    while ((1 << SL) >> b) > lines:
        b += 1
    return b


def plan(vt, rows, nrecs, tail_cut=False):
    """The fields of dml_sparse_plan_info for one chunk (FIELDS)."""
    nrecs = [int(n) for n in nrecs]
    nb, nrec = len(nrecs), sum(nrecs)
    assert 1 <= nb <= K_MAX_W and rows >= 1
    # 1029-1033: leaves of ~kSpLeafCap/2 records on average (double arithmetic, as the C++),
    # at most 65536 leaves
    span = float(K_LEAF_CAP // 2) * float(rows) / float(max(nrec, 1))
    SL = 0
    while SL < 31 and float(1 << (SL + 1)) <= span:
        SL += 1
    while SL < 31 and _cdiv_pow2(rows, SL) > 65536:
        SL += 1
    p = dict(nrec=nrec, **plan_leaves(nrec, rows, SL))
    # 1081-1083 (dml_store.hip:251)
    p["compact"] = int(vt == F32 and p["SL"] + p["D2"] <= K_COMPACT_ROW_BITS and not tail_cut)
    p.update(big=0, BL=0, nbig=0, capS=0)
    big = _plan_big(p, rows, nrecs)
    if big:
        p.update(big=1, **big)
    p["bshift"] = leaf_bshift(p["BL"] if p["big"] else p["SL"])      # 1297 / 1309
    return p


def _plan_big(p, rows, nrecs):
    """1046-1079: BL, nbig, capS when the one-level partition takes the chunk, else None."""
    nb, nrec = len(nrecs), p["nrec"]
    if not p["compact"] or nb < K_SLICES or nrec <= 0:               # 1048
        return None
    BL = 0
    while BL < 24 and _cdiv_pow2(rows, BL) > K_BIG_BINS:             # 1050
        BL += 1
    nbig = _cdiv_pow2(rows, BL)
    mean = nrec // nbig
    if BL > 24 or mean < K_BIG_CAP // 6 or mean > K_BIG_CAP * 17 // 24:  # 1054
        return None
    if BL < p["SL"]:                                                 # 1058
        return None
    srec = [0] * K_SLICES
    for b, n in enumerate(nrecs):
        srec[b % K_SLICES] += n                                      # 1063
    smax = max(srec)
    if smax * K_SLICES > nrec * 5 // 4:                              # 1070
        return None
    capS = 2 * (smax // nbig) + 512                                  # 1076
    if capS >= 0xFFFF:                                               # 1077
        return None
    return dict(BL=BL, nbig=nbig, capS=capS)


def row_index(keys, first, rows):
    """dml_device.h:82-85: the reference's (int)(key - first); -1 outside the shard."""
    d = (np.asarray(keys, np.int64) - np.int64(first)).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    idx = d.astype(np.int64)
    idx = np.where(idx >= 1 << 31, idx - (1 << 32), idx)
    return np.where((idx >= 0) & (idx < rows), idx, -1)


def kernel_name(vt, compact, big):
    """launch_sparse_leaf (1296, 1310-1313)."""
    if big:
        return "dml::k_sp_leaf_big"
    if vt == F64:
        return "dml::k_sp_leaf<double, false>"
    if vt == I32:
        return "dml::k_sp_leaf<int, false>"
    return "dml::k_sp_leaf<float, true>" if compact else "dml::k_sp_leaf<float, false>"


def _over(ids, cap):
    """ids whose count exceeds cap: {id: count}."""
    u, n = np.unique(ids, return_counts=True)
    return {int(a): int(c) for a, c in zip(u, n) if c > cap}


def route(vt, first, rows, pushes_keys, cut=None, tail=None):
    """One chunk's route. pushes_keys: the keys of each push's complete records (<= 64 pushes);
    cut: the (push, record) of the chunk's cutoff, None = the first record whose key lies outside
    the shard, if any; tail: the push that ends inside a record (plan_bucket, dml_store.hip:105-124:
    its tail cut is the position behind its last complete record), None = no push does."""
    nrecs = [len(k) for k in pushes_keys]
    p = plan(vt, rows, nrecs, tail_cut=tail is not None)
    base = np.concatenate([[0], np.cumsum(nrecs)]).astype(np.int64)  # SpPlan::rec_base (1021)
    row = np.concatenate([row_index(k, first, rows) for k in pushes_keys]) if sum(nrecs) else np.zeros(0, np.int64)
    push = np.repeat(np.arange(len(nrecs)), nrecs)
    seq = np.arange(len(row), dtype=np.int64)
    if cut is None:
        bad = np.flatnonzero(row < 0)
        seq_cut = int(bad[0]) if len(bad) else None                  # min pos = first in (push, record) order
    else:
        seq_cut = int(base[cut[0]] + cut[1])                         # sparse_seq_cut (1097-1104)
    if tail is not None:                                             # dml_store.hip:280: the earlier of the two
        seq_cut = min(int(base[tail + 1]), seq_cut if seq_cut is not None else 1 << 62)
    keep = row >= 0                                                  # 621-624: only these take a slot
    row, push, seq = row[keep], push[keep], seq[keep]
    applied = seq < seq_cut if seq_cut is not None else np.ones(len(row), bool)
    SL, D2 = p["SL"], p["D2"]
    leaf = row >> SL
    out = dict(plan=p, big=bool(p["big"]), compact_at_launch=bool(p["compact"]), seq_cut=seq_cut)
    # ---- the single-pass partition's overflow (SpStat::overflow) and the cutoff of compact words
    why = {}
    if p["big"]:
        o = _over((row >> p["BL"]) * K_SLICES + push % K_SLICES, p["capS"])
        if o:
            why["capS"] = o
    else:
        o1, o2 = _over(leaf >> D2, p["cap1"]), _over(leaf, p["cap2"])
        if o1:
            why["cap1"] = o1
        if o2:
            why["cap2"] = o2
    if p["compact"] and seq_cut is not None:                         # dml_store.hip:281
        why["compact_cut"] = seq_cut
    counted = bool(why)
    big, compact = (False, False) if counted else (bool(p["big"]), bool(p["compact"]))  # dml_store.hip:285-287
    out.update(counted=counted, why=why)
    # ---- flagged leaves of the layout the leaf kernel reads
    if big:
        lid, cap, bsh, lsh = row >> p["BL"], K_BIG_CAP, leaf_bshift(p["BL"]), p["BL"]
    else:
        lid, cap, bsh, lsh = leaf, K_LEAF_CAP, leaf_bshift(SL), SL
    flagged = {}
    for L, n in _over(lid, cap).items():
        flagged.setdefault(L, []).append(("records", n))
    bucket = (lid << 32) | ((row - (lid << lsh)) >> bsh)
    ub, inv, cnt = np.unique(bucket, return_inverse=True, return_counts=True)
    hit = np.zeros(len(ub), bool)
    hit[inv[applied]] = True                                         # 488: only an applied record checks
    for b in np.flatnonzero(hit & (cnt > K_BUCKET_MAX)):
        L = int(ub[b] >> 32)
        if not any(r[0] == "records" for r in flagged.get(L, [])):   # 404-410 returns before the buckets
            flagged.setdefault(L, []).append(("bucket", int(cnt[b])))
    if compact:
        rp = (row << 6) | push                                       # the compact word's key (338-339)
        u, n = np.unique(rp, return_counts=True)
        for L in np.unique((u[n > 1] >> 6) >> lsh):
            if not any(r[0] == "records" for r in flagged.get(int(L), [])):
                flagged.setdefault(int(L), []).append(("row_twice_in_push", 1))
    out["flagged"] = flagged
    # ---- sparse_replay's branch (1346-1393)
    if not flagged:
        branch = None
    elif big:
        branch = 1
    elif compact:
        branch = 2
    elif not counted:
        branch = 3
    else:
        branch = 4
    out["replay_branch"] = branch
    out["kernel"] = kernel_name(vt, compact, big)
    out["counters"] = dict(sparse_big_chunks=int(big), sparse_counted_chunks=int(counted),
                           sparse_replays=int(bool(flagged)))
    return out


def predicates(r):
    """The yes/no decisions of a route, for boundary pairs: two members differ in exactly one."""
    kinds = {k for v in r["flagged"].values() for k, _ in v}
    return dict(big=r["big"], compact_at_launch=r["compact_at_launch"], cap1="cap1" in r["why"],
                cap2="cap2" in r["why"], capS="capS" in r["why"], compact_cut="compact_cut" in r["why"],
                leaf_records="records" in kinds, bucket="bucket" in kinds,
                row_twice="row_twice_in_push" in kinds)


# ---- whole push calls: what an existing test's encoded pushes plan ------------------------------
def decode_keys(push, K, stride, V):
    """(keys of the records plan_bucket counts, ragged) of one encoded array push
    (dml_store.hip:105-124): a tail of at least K + V bytes is a readable record
    (FloatArrayStore's 8-byte slots), a shorter one a truncated access."""
    push = bytes(push)
    nfull, tail = divmod(len(push), stride)
    nrec = nfull + (1 if tail >= K + V else 0)
    raw = np.frombuffer(push + b"\0" * stride, np.uint8)[:nrec * stride].reshape(nrec, stride)
    keys = raw[:, :K].copy().view("<i4" if K == 4 else "<i8").ravel().astype(np.int64)
    return keys, 0 < tail < K + V


def call_routes(vt, kt, first, rows, pushes, value_stride=None):
    """route() of every chunk one push call launches (run_batch, dml_store.hip:576-644: chunks of
    kMaxW pushes, a chunk of empty pushes is skipped), up to and including the first chunk that
    meets a cutoff: the store stops there."""
    K = 4 if kt == 0 else 8
    V = 8 if vt == F64 else 4
    stride = K + (value_stride or V)
    out = []
    for c0 in range(0, len(pushes), K_MAX_W):
        dec = [decode_keys(p, K, stride, V) for p in pushes[c0:c0 + K_MAX_W]]
        ragged = [b for b, d in enumerate(dec) if d[1]]
        if not ragged and max(len(d[0]) for d in dec) == 0:
            continue
        out.append(route(vt, first, rows, [d[0] for d in dec], tail=ragged[0] if ragged else None))
        if out[-1]["seq_cut"] is not None:
            break
    return out


def expect(routes):
    """(summed counters, kernel name of the last chunk launched) of call_routes' chunks."""
    keys = ("sparse_big_chunks", "sparse_counted_chunks", "sparse_replays")
    return {k: sum(r["counters"][k] for r in routes) for k in keys}, routes[-1]["kernel"]

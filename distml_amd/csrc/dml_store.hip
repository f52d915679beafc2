// dml_store.hip — host implementation of the C-ABI in include/distml_ps.h.
//
// One dml_store = one DataStore shard (DataStore.java:17-38) resident in HBM on
// one device, with its own HIP stream, a mutex (the reference calls a store
// from three threads: PSAgent.java:278, PSActor.java:171-251, PSSync.java:131),
// and a workspace: [Ctrl | slot table rows x kMaxW int32].
//
// A push batch runs per chunk of <= kMaxW pushes:
//   memset(Ctrl+slots) -> k_index -> k_reduce (matrix)   or
//   memset(Ctrl) -> two-level partition by leaf -> k_sp_leaf (array; dml_sparse.hip)
// and is "retired" later (next call, flush, or immediately in sync mode):
// sync, read Ctrl, replay pushes that repeat a row (exact layered path), undo
// int32 adds past the first negative counter (exact mod 2^32), and turn the
// first failing position into the status code, key and column the reference's
// exception carries.
//
// Also here: the thread-local error string (dml_last_error, dml::set_error), the sticky
// error state and the three device verdicts that feed it (collect_*). The rest of the store
// is dml_store_io.hip, dml_store_owner.hip and dml_store_diag.hip (map: dml_store_impl.h). The
// sharded path's pre-reduce engine (dml_reduce_buckets_dense, dml_prereduce_*, dml_prectx_*) is
// dml_prereduce.hip; what the host translation units share (HIPCHK, DeviceGuard, the push
// tallies) is dml_host.h.
#include "dml_store_impl.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <unordered_map>

using namespace dml;
using namespace dml::detail;

constexpr size_t kSmallStoreBytes = (size_t)1 << 20;  // shards up to 1 MiB: high-priority streams

static thread_local std::string g_err;

int dml::set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

std::pair<hipEvent_t, hipEvent_t> dml::detail::ev_pair(dml_store* s) {
    if (!s->ev_free.empty()) {
        auto p = s->ev_free.back();
        s->ev_free.pop_back();
        return p;
    }
    std::pair<hipEvent_t, hipEvent_t> p{nullptr, nullptr};
    (void)hipEventCreate(&p.first);
    (void)hipEventCreate(&p.second);
    return p;
}

// Collect elapsed times of the completed event pairs (recorded in stream order:
// stop at the first pair still in flight).
void dml::detail::ev_collect(dml_store* s) {
    size_t i = 0;
    for (; i < s->ev_used.size(); ++i) {
        auto& p = s->ev_used[i];
        if (hipEventQuery(p.second) != hipSuccess) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
            s->timed_ms += ms;
            s->timed_n += 1;
        }
        bool ring = false;
        for (const Workspace& W : s->ws) ring |= p.first == W.kstart;
        if (!ring) s->ev_free.push_back(p);
    }
    s->ev_used.erase(s->ev_used.begin(), s->ev_used.begin() + (std::ptrdiff_t)i);
}

int dml::detail::record_error(dml_store* s, int code, int64_t key, int32_t col) {
    if (!s->err) {
        s->err = code;
        s->err_key = key;
        s->err_col = col;
    }
    static const char* names[] = {"", "IllegalArgumentException", "ArrayIndexOutOfBoundsException (key outside shard)",
                                  "ArrayIndexOutOfBoundsException (truncated push)", "IllegalStateException (negative counter)"};
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: key=%lld col=%d", names[code], (long long)key, col);
    return set_err(code, buf);
}

namespace {

int ensure_stage(dml_store* s, size_t bytes) {
    if (bytes <= s->stage_cap) return DML_OK;
    if (s->hstage) (void)hipHostFree(s->hstage);
    if (s->dstage) (void)hipFree(s->dstage);
    s->hstage = nullptr;
    s->dstage = nullptr;
    s->stage_cap = 0;
    size_t cap = std::max<size_t>(bytes, 1 << 20);
    HIPCHK(hipHostMalloc((void**)&s->hstage, cap, hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&s->dstage, cap));
    s->stage_cap = cap;
    return DML_OK;
}

// Per-push record accounting: records with a complete key, and the position of
// the first truncated access of a ragged tail (DataDesc.readInt past data.length).
void plan_bucket(const dml_store* s, int64_t len, int gb, int64_t* nrec, uint64_t* tail_cut) {
    const int64_t nfull = len / s->stride, tail = len % s->stride;
    *nrec = nfull;
    *tail_cut = kNoPos;
    if (tail == 0) return;
    const int64_t t0 = nfull * s->stride;
    if (s->is_matrix) {
        if (tail < s->K) {
            *tail_cut = pos_of((uint64_t)gb, (uint64_t)t0);
        } else {
            *nrec = nfull + 1;  // key complete: the index sees it (an out-of-shard key is reported first)
            const int64_t nvals = (tail - s->K) / s->V;
            *tail_cut = pos_of((uint64_t)gb, (uint64_t)(t0 + s->K + nvals * s->V));
        }
    } else if (tail >= s->K + s->V) {
        *nrec = nfull + 1;  // readable record (FloatArrayStore 8-byte stride, short last slot)
    } else {
        *tail_cut = pos_of((uint64_t)gb, (uint64_t)t0);
    }
}

// Apply part of a chunk on the main stream (after its index is ready), then
// copy its Ctrl out and record `done`. `prev` = Ctrl of the chunk enqueued before.
int launch_apply(dml_store* s, Chunk& c, Workspace& W, const Ctrl* prev) {
    c.bt.prev = prev;
    g_kernel_name = nullptr;
    struct NameOnExit {
        dml_store* s;
        ~NameOnExit() {
            if (g_kernel_name) s->kname = g_kernel_name;
        }
    } name_on_exit{s};
    if (s->is_matrix) {
        // Boundary between consecutive reduces (measured): the chunk's
        // completion event rides in the reduce's dispatch packet (a marker packet after
        // it cost ~7 µs); a timed chunk also carries its start event there (start/stop
        // in every packet ~10 µs, so the bench times a sample of the chunks). AdaGrad's
        // finalize kernels follow the reduce: marker events around both.
        const bool inpacket = !s->adagrad;
        const bool timed = s->timing && (s->adagrad || s->timing_every <= 1 || s->timing_k++ % s->timing_every == 0);
        LaunchEv ev = inpacket ? LaunchEv{timed ? W.kstart : nullptr, W.applied} : LaunchEv{};
        if (timed && !inpacket) HIPCHK(hipEventRecord(W.kstart, s->stream));
        int64_t nblk = 0;
        W.clears = reduce_clears_slots(vtype_of(s->desc), reduce_mode(s), s->cols);
        c.bt.src = c.in != c.out ? c.in : nullptr;
        if (W.flat_ident) s->st.ident_launches += 1;
        if (W.flat_ident && s->adagrad)  // every push verified-identity (the host's Ctrl copy)
            HIPCHK(launch_ada_ident(c.out, s->rows, s->cols, c.bt, c.nb, s->stride, s->K, ada_args(s), s->stream,
                                    &nblk, ev));
        else if (W.flat_ident)
            HIPCHK(launch_flat_ident(vtype_of(s->desc), reduce_mode(s), c.out, s->rows, s->cols, c.bt, c.nb,
                                     s->stride, s->K, W.ctrl, s->stream, &nblk, ev));
        else
            HIPCHK(launch_reduce(vtype_of(s->desc), reduce_mode(s), c.out, s->rows, s->cols, c.bt, c.nb, s->stride,
                                 s->K, W.slot, W.rowflag, W.ctrl, c.tail_cut, ada_args(s), s->stream, &nblk, ev));
        if (s->adagrad)
            // finalized here unless the index saw a repeated row: then after its replay
            HIPCHK(launch_maxdelta_finalize(s->cand, nblk, s->md, c.bt, c.nb, s->stride, s->K, s->V, s->stream,
                                            kMdDeferIfRepeat, W.ctrl));
        if (!inpacket || nblk <= 0) HIPCHK(hipEventRecord(W.applied, s->stream));  // (no dispatch: a marker)
        if (timed && nblk > 0) s->ev_used.emplace_back(W.kstart, W.applied);
    } else {
        // the leaf launch carries the chunk's completion event (and, when timed, its start)
        const bool launched = c.sp.nleaves > 0;
        const bool timed = launched && s->timing && (s->timing_every <= 1 || s->timing_k++ % s->timing_every == 0);
        const LaunchEv ev = launched ? LaunchEv{timed ? W.kstart : nullptr, W.applied} : LaunchEv{};
        HIPCHK(launch_sparse_leaf(vtype_of(s->desc), s->data, c.sp, c.spl, W.sp, W.ctrl, prev, s->stream, ev));
        if (!launched) HIPCHK(hipEventRecord(W.applied, s->stream));
        if (timed) s->ev_used.emplace_back(W.kstart, W.applied);
    }
    // ctrl read-back on its own stream, so the next chunk's apply follows this one directly
    HIPCHK(hipStreamWaitEvent(s->cstream, W.applied, 0));
    HIPCHK(hipMemcpyAsync(W.hctrl, W.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s->cstream));
    HIPCHK(hipEventRecord(W.done, s->cstream));
    return DML_OK;
}

// Index on the side stream (overlaps the previous chunk's apply), then apply.
int launch_chunk(dml_store* s, Chunk& c, Workspace& W, const Ctrl* prev) {
    hipStream_t is = s->istream;
    // A workspace whose last chunk retired normally through a slot-clearing reduce
    // (k_reduce_rows, plain-sum modes) already holds an all -1 slot table and zero
    // rowflags: only its Ctrl is reset (the 4 MiB-class memsets otherwise compete
    // with the running reduce).
    const bool clean = W.clean, kept = W.kept;
    W.clean = W.kept = false;
    // A speculative chunk after a kept table needs no -1 table either: its pushes
    // are full-range, so the index rewrites every row of each column it builds (a
    // push that is no permutation fails the chunk's verification, and the re-run
    // starts from a memset), and identity / reused columns are not rebuilt.
    const bool slots_ok = clean || (kept && c.keeps);
    HIPCHK(hipMemsetAsync(W.base, 0xFF, sizeof(Ctrl) + (slots_ok ? 0 : s->slot_bytes), is));
    if (s->is_matrix) {
        if (!(clean || kept)) HIPCHK(hipMemsetAsync(W.rowflag, 0, (size_t)s->rows * sizeof(uint32_t), is));
        if (c.spec) {
            HIPCHK(launch_ident_check(c.bt, c.nb, s->stride, s->K, s->first, s->rows, W.slot, W.ctrl, is));
            // pushes matched to kept columns: the indexed ones take columns nobody reads
            if (c.bt.kept_cols) HIPCHK(launch_assign_cols(W.ctrl, c.nb, is));
        }
        // AdaGrad chunks of k_ada_flat (no speculation: the apply cannot be undone):
        // full-range pushes whose records are rows in order skip the key index after a
        // complete key check, when the slot table is beyond the caches (its atomics go
        // to DRAM; see prereduce_begin_tail, dml_prereduce.hip)
        c.bt.ident_ok = 0;
        if (s->adagrad && c.tail_cut == kNoPos &&
            use_flat(vtype_of(s->desc), reduce_mode(s), s->cols, c.bt, c.nb, s->rows) &&
            full_range_beyond_caches(c.bt, c.nb, s->rows, s->ident_full_min)) {
            HIPCHK(launch_ident_full(c.bt, c.nb, c.max_nrec, s->stride, s->K, s->first, s->rows, W.ctrl, is));
            c.bt.ident_ok = 1;
        }
        // Sparse-row chunks of k_reduce_rows (some push lists only part of the rows): the
        // index marks the rows any push lists, and the reduce skips the others' shard rows
        c.bt.listed = nullptr;
        if (!c.spec && !s->adagrad && (reduce_mode(s) == kAdd || reduce_mode(s) == kAddCheckI32) &&
            !use_flat(vtype_of(s->desc), reduce_mode(s), s->cols, c.bt, c.nb, s->rows)) {
            bool part = false;
            for (int j = 0; j < c.nb && !part; ++j) part = c.bt.nrec[j] < s->rows;
            if (part) {
                if (!W.listed) HIPCHK(hipMalloc((void**)&W.listed, (size_t)s->rows));
                HIPCHK(hipMemsetAsync(W.listed, 0, (size_t)s->rows, is));
                c.bt.listed = W.listed;
            }
        }
        HIPCHK(launch_index(c.bt, c.nb, c.max_nrec, s->stride, s->K, s->first, s->rows, W.slot, W.rowflag, W.ctrl,
                            c.tail_cut, is));
        // A speculative chunk of the flat shape: its Ctrl (identity / kept columns,
        // cutoff, repeats) is final here; a pinned copy lets the host pick the lean
        // all-identity kernel after the wait below (k_flat_ident)
        W.flat_ident = false;
        // AdaGrad chunks checked record by record (ident_ok) likewise pick k_ada_ident
        if (((c.spec && reduce_mode(s) == kAdd) || (s->adagrad && c.bt.ident_ok)) &&
            c.tail_cut == kNoPos && use_flat(vtype_of(s->desc), reduce_mode(s), s->cols, c.bt, c.nb, s->rows)) {
            if (!W.hidx) HIPCHK(hipHostMalloc((void**)&W.hidx, sizeof(Ctrl), hipHostMallocDefault));
            W.hidx->cutoff = 0;  // not all-identity unless the copy lands
            HIPCHK(hipMemcpyAsync(W.hidx, W.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, is));
            W.flat_ident = true;  // provisional: decided after idx_done
        }
    } else {
        // arrays: partition the chunk by leaf (row range) for the ordered per-leaf
        // apply (its first pass also finds the cutoff); int32 leaves check every add
        // (IntArrayStore.java:108-110) and report the chunk's first negative counter
        const int vt = vtype_of(s->desc);
        c.sorted = true;
        {
            c.sp = sparse_plan(c.bt, c.nb, s->rows);
            // one 8-B word per fp32 record through the partition
            c.sp.compact = sparse_compact_ok(vt, c.sp, c.tail_cut != kNoPos);
            // big leaves sorted in LDS where they apply: no second partition pass (§4)
            sparse_plan_big(c.sp, c.bt, s->rows);
            c.spl = sparse_layout(c.sp, s->V);
            if (W.sp_cap < c.spl.total) {
                HIPCHK(hipStreamSynchronize(s->stream));  // W's previous chunk is retired; be safe
                (void)hipFree(W.sp);
                W.sp = nullptr;
                W.sp_cap = 0;
                HIPCHK(hipMalloc((void**)&W.sp, c.spl.total));
                W.sp_cap = c.spl.total;
            }
            if (!W.hsp) HIPCHK(hipHostMalloc((void**)&W.hsp, sizeof(SpStat), hipHostMallocDefault));
            if (c.sp.big)
                HIPCHK(launch_sparse_partition_big(c.bt, c.sp, c.spl, W.sp, s->stride, s->K, s->first, s->rows,
                                                   W.ctrl, c.tail_cut, W.hsp, is));
            else
                HIPCHK(launch_sparse_partition_fast(vt, c.bt, c.sp, c.spl, W.sp, s->stride, s->K, s->first, s->rows,
                                                    W.ctrl, c.tail_cut, W.hsp, is));
        }
    }
    HIPCHK(hipEventRecord(W.idx_done, is));
    // The index (tens of µs) finishes while the previous chunk's reduce (hundreds
    // of µs) still runs: wait for it on the host and enqueue this chunk's apply
    // directly behind that reduce. A cross-queue barrier packet instead costs
    // ~16 µs of idle GPU between the two reduces (measured).
    HIPCHK(hipEventSynchronize(W.idx_done));
    if (W.flat_ident) W.flat_ident = flat_ident_ok(*W.hidx, c.bt, c.nb, s->rows, c.tail_cut);
    if (c.sorted && c.sp.fast) {
        const uint64_t pcut = std::min<uint64_t>(W.hsp->cutoff, c.tail_cut);
        if (W.hsp->overflow || (c.sp.compact && pcut != kNoPos)) {
            // a bin or leaf of the single-pass partition overflowed (skewed keys), or
            // compact records met a cutoff (they carry no sequence to cut at): the
            // counted partition, compact layout (still beside the running apply)
            c.sp.fast = 0;
            c.sp.compact = 0;
            c.sp.big = 0;
            c.sp.seq_cut = kSpSkip;
            HIPCHK(launch_sparse_partition(vtype_of(s->desc), c.bt, c.sp, c.spl, W.sp, s->stride, s->K, s->first,
                                           s->rows, W.ctrl, c.tail_cut, is));
            HIPCHK(hipEventRecord(W.idx_done, is));
            HIPCHK(hipEventSynchronize(W.idx_done));
        } else {
            c.sp.seq_cut = sparse_seq_cut(c.sp, c.bt, pcut, s->stride);
        }
    }
    return launch_apply(s, c, W, prev);
}

int read_ctrl(dml_store* s, Workspace& W, Ctrl* out) {
    HIPCHK(hipMemcpyAsync(W.hctrl, W.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    *out = *W.hctrl;
    return DML_OK;
}

// Exact replay of the rows some push lists twice (rowflag set; the reduce left
// them untouched): split each push into layers (k-th occurrence of each flagged
// row) and apply layers in (push, layer) order, so per element the adds keep
// their reference order. Other rows are final already (rows are independent).
int replay_rows(dml_store* s, const Chunk& c, Workspace& W, Ctrl* ctl) {
    std::vector<uint32_t> flag((size_t)s->rows);
    HIPCHK(hipMemcpyAsync(flag.data(), W.rowflag, flag.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    struct VCol { int src_b; std::vector<std::pair<int32_t, int32_t>> rr; };
    std::vector<VCol> cols;
    int32_t* drows = nullptr;
    HIPCHK(hipMalloc((void**)&drows, sizeof(int32_t) * std::max<int64_t>(c.max_nrec, 1)));
    std::vector<int32_t> hrows;
    for (int b = 0; b < c.nb; ++b) {
        const int64_t n = c.bt.nrec[b];
        hrows.resize((size_t)n);
        if (n > 0) {
            hipError_t e = launch_key_rows(c.bt.base[b], n, s->stride, s->K, s->first, s->rows, drows, s->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hrows.data(), drows, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
            if (e != hipSuccess) { (void)hipFree(drows); return set_err(DML_E_HIP, hipGetErrorString(e)); }
        }
        std::unordered_map<int32_t, int32_t> occ;
        std::vector<VCol> layers;
        for (int64_t r = 0; r < n; ++r) {
            const int32_t row = hrows[(size_t)r];
            if (row < 0 || !flag[(size_t)row]) continue;  // out of shard (cutoff covers it) or already applied
            const int32_t l = occ[row]++;
            if ((int)layers.size() <= l) layers.push_back(VCol{b, {}});
            layers[(size_t)l].rr.emplace_back(row, (int32_t)r);
        }
        for (auto& L : layers) cols.push_back(std::move(L));
    }
    (void)hipFree(drows);
    std::vector<int32_t> hslot((size_t)s->rows * kMaxW);
    auto upload = [&](size_t v0, Chunk& vc) -> int {
        vc.nb = (int)std::min<size_t>(kMaxW, cols.size() - v0);
        vc.tail_cut = c.tail_cut;
        vc.bt.prev = nullptr;
        std::fill(hslot.begin(), hslot.end(), -1);
        for (int j = 0; j < vc.nb; ++j) {
            const VCol& col = cols[v0 + (size_t)j];
            vc.bt.base[j] = c.bt.base[col.src_b];
            vc.bt.len[j] = c.bt.len[col.src_b];
            vc.bt.nrec[j] = c.bt.nrec[col.src_b];
            vc.bt.bidx[j] = c.bt.bidx[col.src_b];
            for (auto& pr : col.rr) hslot[(size_t)pr.first * (size_t)slot_stride(vc.nb) + (size_t)j] = pr.second;
        }
        HIPCHK(hipMemcpy(W.slot, hslot.data(), hslot.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return DML_OK;
    };
    for (size_t v0 = 0; v0 < cols.size(); v0 += kMaxW) {
        Chunk vc;
        if (int rc = upload(v0, vc)) return rc;
        int64_t nblk = 0;
        HIPCHK(launch_reduce(vtype_of(s->desc), reduce_mode(s), s->data, s->rows, s->cols, vc.bt, vc.nb, s->stride,
                             s->K, W.slot, nullptr, W.ctrl, vc.tail_cut, ada_args(s), s->stream, &nblk));
        if (s->adagrad)  // the layers' candidates join the chunk's pending one
            HIPCHK(launch_maxdelta_finalize(s->cand, nblk, s->md, vc.bt, vc.nb, s->stride, s->K, s->V, s->stream,
                                            kMdDefer));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (s->adagrad) {  // one finalize over the whole chunk: the reference's first position wins a tie
        HIPCHK(launch_maxdelta_finalize(s->cand, 0, s->md, c.bt, c.nb, s->stride, s->K, s->V, s->stream, kMdApply));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (int rc = read_ctrl(s, W, ctl)) return rc;
    if (ctl->neg_pos != kNoPos) {
        // undo every add after the first negative: the unflagged rows (rebuilt slot
        // table of the chunk) and every layer of the replayed rows
        Chunk mc = c;
        mc.bt.prev = nullptr;
        HIPCHK(hipMemsetAsync(W.slot, 0xFF, s->slot_bytes, s->stream));
        HIPCHK(launch_index(mc.bt, mc.nb, mc.max_nrec, s->stride, s->K, s->first, s->rows, W.slot, W.rowflag, W.ctrl,
                            kNoPos, s->stream));
        HIPCHK(launch_rollback_i32((int32_t*)s->data, s->rows, s->cols, mc.bt, mc.nb, s->stride, s->K, W.slot,
                                   W.rowflag, W.ctrl, mc.tail_cut, s->stream));
        for (size_t v0 = 0; v0 < cols.size(); v0 += kMaxW) {
            Chunk vc;
            HIPCHK(hipStreamSynchronize(s->stream));
            if (int rc = upload(v0, vc)) return rc;
            HIPCHK(launch_rollback_i32((int32_t*)s->data, s->rows, s->cols, vc.bt, vc.nb, s->stride, s->K, W.slot,
                                       nullptr, W.ctrl, vc.tail_cut, s->stream));
        }
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    return DML_OK;
}

int64_t read_key_at(dml_store* s, const uint8_t* dev_rec) {
    uint8_t kb[8] = {0};
    if (hipMemcpy(kb, dev_rec, (size_t)s->K, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (s->K == 4) {
        int32_t k;
        std::memcpy(&k, kb, 4);
        return k;
    }
    int64_t k;
    std::memcpy(&k, kb, 8);
    return k;
}

const uint8_t* base_of(const Chunk& c, int gb) {
    for (int b = 0; b < c.nb; ++b)
        if (c.bt.bidx[b] == gb) return c.bt.base[b];
    return nullptr;
}

// A chunk's input and output shard buffers: it reads `in` (the output of the
// chunk before it); a speculative chunk writes the other buffer, so the input
// survives until its identity records are verified.
void set_buffers(dml_store* s, Chunk& c, void* in) {
    c.in = in;
    c.out = c.spec ? (in == s->data ? s->data_alt : s->data) : in;
}

// Failed identity speculation: redo the chunk without it, in place on its input
// (== s->data: every chunk before it has retired), on the apply stream, and
// return the new Ctrl. The workspace's slot table / rowflags are rebuilt.
int rerun_unspeculated(dml_store* s, Chunk& c, Workspace& W, Ctrl* ctl) {
    c.spec = false;
    c.bt.spec = 0;
    c.keeps = false;
    c.bt.kept_cols = 0;
    c.bt.keeps = 0;
    c.bt.prev = nullptr;
    set_buffers(s, c, s->data);
    HIPCHK(hipMemsetAsync(W.base, 0xFF, sizeof(Ctrl) + s->slot_bytes, s->stream));
    HIPCHK(hipMemsetAsync(W.rowflag, 0, (size_t)s->rows * sizeof(uint32_t), s->stream));
    HIPCHK(launch_index(c.bt, c.nb, c.max_nrec, s->stride, s->K, s->first, s->rows, W.slot, W.rowflag, W.ctrl,
                        c.tail_cut, s->stream));
    c.bt.src = nullptr;
    int64_t nblk = 0;
    HIPCHK(launch_reduce(vtype_of(s->desc), reduce_mode(s), c.out, s->rows, s->cols, c.bt, c.nb, s->stride, s->K,
                         W.slot, W.rowflag, W.ctrl, c.tail_cut, ada_args(s), s->stream, &nblk));
    W.clears = reduce_clears_slots(vtype_of(s->desc), reduce_mode(s), s->cols);
    return read_ctrl(s, W, ctl);
}

// Turn the oldest pending chunk's Ctrl into final state + status: replay rows a
// push repeats, undo int32 adds past the first negative counter, map the first
// failing position to (code, key, col). If it ended abnormally, the chunk queued
// after it ran as a no-op: relaunch it (replay only) or drop it (error: the
// reference's PS loop has ended, PSAgent.java:188-191).
int retire_front(dml_store* s) {
    if (s->pend.empty()) return DML_OK;
    Pending p = s->pend.front();
    s->pend.pop_front();
    Workspace& W = s->ws[p.w];
    Chunk& c = p.c;
    HIPCHK(hipEventSynchronize(W.done));
    Ctrl ctl = *W.hctrl;
    if (s->timing) ev_collect(s);
    const bool abnormal = ctrl_abnormal(&ctl);  // the chunk queued behind it ran as a no-op
    W.clean = s->is_matrix && !abnormal && W.clears;
    s->st.chunks += 1;
    if (!s->is_matrix && c.sp.big) s->st.sparse_big_chunks += 1;
    if (!s->is_matrix && !c.sp.fast) s->st.sparse_counted_chunks += 1;  // launch_chunk fell back
    if (c.spec && ctl.spec_ok != 0u) {
        std::swap(s->data, s->data_alt);  // every identity record verified: the output is the shard
        s->st.spec_chunks += 1;
        const uint64_t perm = tally_verified_pushes(ctl, c.nb, s->st);
        if (c.keeps) {  // the reduce left the slot table as built: the next chunk here may reuse it
            W.clean = false;
            W.kept = true;
            W.kept_nb = c.nb;
            W.perm = perm;
        }
    } else if (c.spec) {
        // An identity push was not (or the chunk met a cutoff / repeated row): the
        // output is discarded and the chunk re-runs exactly, in place on its input
        // (the shard as of the chunks before it), with the full key index.
        s->st.spec_chunks += 1;
        s->st.spec_reruns += 1;
        s->st.indexed_pushes += c.nb;
        if (int r2 = rerun_unspeculated(s, c, W, &ctl)) return r2;
        W.clean = !ctrl_abnormal(&ctl) && W.clears;
    } else if (s->is_matrix) {
        // non-speculative: AdaGrad chunks may have skipped the index for pushes checked
        // completely (Batch::ident_ok)
        tally_checked_pushes(ctl, c.nb, c.bt.ident_ok != 0, s->st);
    }
    int rc = DML_OK;
    if (s->is_matrix && ctl.no_dup == 0u) {
        rc = replay_rows(s, c, W, &ctl);
        if (rc) return rc;
    } else if (!s->is_matrix && ctl.no_dup == 0u) {
        // leaves too large for the LDS sort were skipped by the leaf kernel: apply them
        // exactly (an int32 replay may find an earlier negative counter)
        s->st.sparse_replays += 1;
        HIPCHK(sparse_replay(vtype_of(s->desc), s->data, c.sp, c.spl, W.sp, c.bt, s->stride, s->K, s->first, s->rows,
                             W.ctrl, c.tail_cut, s->stream));
        HIPCHK(hipMemcpyAsync(&ctl.neg_pos, &W.ctrl->neg_pos, sizeof(ctl.neg_pos), hipMemcpyDeviceToHost,
                              s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    if (!s->is_matrix && ctl.neg_pos != kNoPos) {
        // int32 array: the leaves reported the sequence of the chunk's first add that left
        // a counter negative; as a position (push, record) it bounds the rollback of every
        // later add (exact mod 2^32), the state the reference leaves when it throws
        const uint64_t seq = ctl.neg_pos;
        int b = 0;
        while (b + 1 < c.nb && (uint64_t)c.sp.rec_base[b + 1] <= seq) ++b;
        const int64_t r = (int64_t)(seq - (uint64_t)c.sp.rec_base[b]);
        ctl.neg_pos = pos_of((uint64_t)c.bt.bidx[b], (uint64_t)(r * s->stride + s->K));
        HIPCHK(hipMemcpyAsync(&W.ctrl->neg_pos, &ctl.neg_pos, sizeof(ctl.neg_pos), hipMemcpyHostToDevice, s->stream));
        for (int j = 0; j < c.nb; ++j)
            HIPCHK(launch_array_rollback_i32((int32_t*)s->data, s->rows, c.bt.base[j], c.bt.nrec[j], c.bt.bidx[j],
                                             s->stride, s->K, s->first, W.ctrl, c.tail_cut, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    } else if (s->is_matrix && ctl.neg_pos != kNoPos && ctl.no_dup != 0u) {
        // (a chunk with repeated rows rolled back inside replay_rows) the reduce handed
        // its slot rows back clean: rebuild the table (no row repeats here, so the
        // rowflags stay zero; the index leaves neg_pos alone), then undo past neg_pos
        HIPCHK(hipMemsetAsync(W.slot, 0xFF, s->slot_bytes, s->stream));
        HIPCHK(launch_index(c.bt, c.nb, c.max_nrec, s->stride, s->K, s->first, s->rows, W.slot, W.rowflag, W.ctrl,
                            c.tail_cut, s->stream));
        HIPCHK(launch_rollback_i32((int32_t*)s->data, s->rows, s->cols, c.bt, c.nb, s->stride, s->K, W.slot, W.rowflag,
                                   W.ctrl, c.tail_cut, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
    }
    const uint64_t cut = std::min<uint64_t>(ctl.cutoff, c.tail_cut);
    if (ctl.neg_pos != kNoPos && ctl.neg_pos < cut) {
        const int gb = (int)(ctl.neg_pos >> 40);
        const int64_t off = (int64_t)(ctl.neg_pos & kOffMask);
        const int64_t r = off / s->stride;
        const int32_t col = s->is_matrix ? (int32_t)((off - r * s->stride - s->K) / s->V) : -1;
        rc = record_error(s, DML_E_NEGATIVE_COUNTER, read_key_at(s, base_of(c, gb) + r * s->stride), col);
    } else if (cut != kNoPos) {
        const int gb = (int)(cut >> 40);
        const int64_t off = (int64_t)(cut & kOffMask);
        const int64_t r = off / s->stride;
        const uint8_t* rec = base_of(c, gb) + r * s->stride;
        if (ctl.cutoff < c.tail_cut) {
            rc = record_error(s, DML_E_KEY_OUT_OF_SHARD, read_key_at(s, rec), -1);
        } else {
            // truncated: the key is known when the record's key bytes were complete
            int64_t len = 0;
            for (int b = 0; b < c.nb; ++b)
                if (c.bt.bidx[b] == gb) len = c.bt.len[b];
            const bool key_ok = len - r * s->stride >= s->K;
            int32_t col = -1;
            if (s->is_matrix && key_ok) col = (int32_t)((off - r * s->stride - s->K) / s->V);
            rc = record_error(s, DML_E_TRUNCATED, key_ok ? read_key_at(s, rec) : 0, col);
        }
    }
    if (abnormal && !s->pend.empty()) {
        if (rc != DML_OK) {
            for (auto& q : s->pend) (void)hipEventSynchronize(s->ws[q.w].done);
            s->pend.clear();  // their kernels were no-ops; the store stops here like the reference
        } else {
            Pending& q = s->pend.front();  // relaunch its apply; its index is still valid
            HIPCHK(hipEventSynchronize(s->ws[q.w].done));
            set_buffers(s, q.c, s->data);
            if (int r2 = launch_apply(s, q.c, s->ws[q.w], nullptr)) return r2;
        }
    }
    return rc;
}

// retire_front for its callers: after an error the store stops, and nothing stays pending.
int retire_one(dml_store* s) {
    const int rc = retire_front(s);
    if (rc) s->pend.clear();
    return rc;
}

// Run `n` device-resident pushes (global indices 0..n-1) as ordered chunks of
// <= kMaxW; up to two chunks stay in flight (retired later, in order).
int run_batch(dml_store* s, const uint8_t* const* dptr, const int64_t* lens, int n) {
    if (int rc = collect_apply_check(s, false)) return rc;  // an int32 owner apply failed earlier
    const uint64_t seq = ++s->call_seq;
    for (int c0 = 0; c0 < n; c0 += kMaxW) {
        Chunk c;
        c.seq = seq;
        c.nb = std::min(kMaxW, n - c0);
        for (int j = 0; j < c.nb; ++j) {
            const int gb = c0 + j;
            int64_t nrec;
            uint64_t tcut;
            plan_bucket(s, lens[gb], gb, &nrec, &tcut);
            c.bt.base[j] = dptr[gb];
            c.bt.len[j] = lens[gb];
            c.bt.nrec[j] = nrec;
            c.bt.bidx[j] = gb;
            c.max_nrec = std::max(c.max_nrec, nrec);
            c.tail_cut = std::min(c.tail_cut, tcut);
        }
        if (c.max_nrec == 0 && c.tail_cut == kNoPos) continue;  // empty pushes: nothing to apply
        while ((int)s->pend.size() >= kRing - 1)  // see kRing
            if (int rc = retire_one(s)) return rc;
        if (int rc = failed(s)) return rc;
        // Identity speculation: plain-sum matrices of the spec_shape
        // widths, when every push of the chunk is full-range (one record per row, no
        // ragged tail): no key index, the reduce verifies every record's key.
        if (s->is_matrix && reduce_mode(s) == kAdd && !s->no_spec && spec_shape(vtype_of(s->desc), s->cols) &&
            c.tail_cut == kNoPos) {
            bool full = true;
            for (int j = 0; j < c.nb && full; ++j) full = c.bt.nrec[j] == s->rows && c.bt.len[j] == s->rows * s->stride;
            if (full && !s->data_alt) {
                // the second shard buffer, only with headroom left for the caller's
                // buffers (exchange slices, partials): 1/8 of the device or 4 GiB
                const size_t need = (size_t)s->rows * (size_t)s->cols * (size_t)s->V;
                size_t free_b = 0, total_b = 0;
                const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
                                  free_b > need + std::max<size_t>(total_b / 8, (size_t)4 << 30);
                if (!room || hipMalloc(&s->data_alt, need) != hipSuccess) {
                    (void)hipGetLastError();
                    s->data_alt = nullptr;
                    s->no_spec = true;  // no room for a second buffer: no speculation
                }
            }
            c.spec = full && s->data_alt;
        }
        c.bt.spec = c.spec ? 1 : 0;
        // Slot reuse: a speculative chunk may take a push's slots from
        // any column its workspace kept (a verified permutation of the workspace's
        // previous chunk), when that push's sampled keys match it (k_ident_check)
        c.bt.kept_cols = 0;
        c.keeps = c.spec;
        c.bt.keeps = c.keeps ? 1 : 0;
        if (c.keeps) {
            const Workspace& Wn = s->ws[s->next_ws];
            if (Wn.kept && slot_stride(Wn.kept_nb) == slot_stride(c.nb)) c.bt.kept_cols = Wn.perm;
        }
        c.bt.first = s->first;
        const Ctrl* prev = s->pend.empty() ? nullptr : s->ws[s->pend.back().w].ctrl;
        set_buffers(s, c, s->pend.empty() ? s->data : s->pend.back().c.out);
        Pending p;
        p.c = c;
        p.w = s->next_ws;
        s->next_ws = (s->next_ws + 1) % kRing;
        int rc = launch_chunk(s, p.c, s->ws[p.w], prev);
        if (rc) return rc;
        s->pend.push_back(p);
    }
    return DML_OK;
}

}  // namespace

int dml::detail::retire_all(dml_store* s) {
    while (!s->pend.empty())
        if (int rc = retire_one(s)) return rc;
    return DML_OK;
}

// A chained int32 commit that brought a closed record home: the store's IllegalStateException
// with the record's key and column. The device record stays closed (k_chain_i32_merge keeps
// the first verdict) until dml_store_clear_error.
int dml::detail::collect_chain_check(dml_store* s, bool block) {
    ChainI32Rec r;
    if (int rc = s->crec.poll(block, &r)) return rc;
    if (r.pos == kNoPos) return DML_OK;
    return record_error(s, DML_E_NEGATIVE_COUNTER, (int64_t)r.key, r.col);
}

// Verdict of the device list fetches (dml_store_fetch_device): the first key outside the
// shard becomes the store's ArrayIndexOutOfBoundsException, as the host fetch's does. Unlike
// the other two, a reported verdict reopens its device record at once, behind the fetches
// launched so far.
int dml::detail::collect_fetch_check(dml_store* s, bool block) {
    FetchVerdict v;
    if (int rc = s->fver.poll(block, &v)) return rc;
    if (v.idx == kNoPos) return DML_OK;
    if (int rc = s->fver.reopen(s->stream)) return rc;
    return record_error(s, DML_E_KEY_OUT_OF_SHARD, v.key, -1);
}

// Chain, then fetch, then the int32 owner applies (dml_store_apply_dense_device), whose first
// negative final counter is the store's IllegalStateException and, like the chain's record,
// stays closed until dml_store_clear_error: the first error returns.
int dml::detail::collect_apply_check(dml_store* s, bool block) {
    if (int rc = collect_chain_check(s, block)) return rc;
    if (int rc = collect_fetch_check(s, block)) return rc;
    unsigned long long idx;
    if (int rc = s->neg.poll(block, &idx)) return rc;
    if (idx == kNoPos) return DML_OK;
    return record_error(s, DML_E_NEGATIVE_COUNTER, s->first + (int64_t)(idx / (unsigned long long)s->cols),
                        (int32_t)(idx % (unsigned long long)s->cols));
}

int dml::detail::begin_call(dml_store* s) {
    int rc = retire_all(s);
    int rc2 = collect_apply_check(s, true);
    return rc ? rc : rc2;
}

// ===========================================================================
extern "C" {

const char* dml_last_error(void) { return g_err.c_str(); }
const char* dml_version(void) { return "distml_amd 0.1 (gfx950)"; }

int dml_linear_split(int64_t first_key, int64_t last_key, int32_t n, int64_t* first_out, int64_t* last_out) {
    if (n <= 0 || !first_out || !last_out) return set_err(DML_E_INVALID_ARG, "bad linear_split args");
    // KeyRange.linearSplit (KeyRange.java:68-80)
    int64_t start = first_key;
    const int64_t step = (last_key - first_key + n) / n;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t end = std::min(start + step - 1, last_key);
        first_out[i] = start;
        last_out[i] = end;
        start += step;
    }
    return DML_OK;
}

int dml_store_create_range(const dml_desc* desc, int64_t first_key, int64_t last_key, int32_t cols, int32_t device,
                           uint32_t flags, dml_store** out) {
    if (!desc || !out) return set_err(DML_E_INVALID_ARG, "null argument");
    *out = nullptr;
    const dml_desc d = *desc;
    // DataStore.createStore dispatch (DataStore.java:50-92)
    if ((d.data_type != 0 && d.data_type != 1) || (d.key_type != 0 && d.key_type != 1) ||
        (d.value_type != DML_ELEMENT_TYPE_INT && d.value_type != DML_ELEMENT_TYPE_FLOAT &&
         d.value_type != DML_ELEMENT_TYPE_DOUBLE))
        return set_err(DML_E_BAD_DESC, "Unrecognized matrix type (DataStore.createStore)");
    if (d.data_type == 1 && !d.dense_column)
        return set_err(DML_E_UNSUPPORTED, "sparse-column matrix pushes are not supported (SURVEY defect 3)");
    if (last_key < first_key) return set_err(DML_E_INVALID_ARG, "empty KeyRange shard");
    if (d.data_type == 1 && cols <= 0) return set_err(DML_E_INVALID_ARG, "cols must be > 0");
    const int64_t rows = last_key - first_key + 1;
    if (rows > INT32_MAX) return set_err(DML_E_INVALID_ARG, "shard larger than a Java array");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return set_err(DML_E_HIP, "no HIP device");
    if (device < 0 || device >= ndev) return set_err(DML_E_INVALID_ARG, "bad device ordinal");
    DeviceGuard g(device);

    auto* s = new (std::nothrow) dml_store();
    if (!s) return set_err(DML_E_NOMEM, "out of host memory");
    s->device = device;
    s->desc = d;
    s->flags = flags;
    s->no_spec = (flags & DML_FLAG_NO_SPECULATION) != 0;
    s->is_matrix = d.data_type == 1;
    s->adagrad = s->is_matrix && d.value_type == DML_ELEMENT_TYPE_FLOAT && d.ada_grad;
    s->K = desc_key_bytes(d);
    s->V = (d.value_type == DML_ELEMENT_TYPE_INT || d.value_type == DML_ELEMENT_TYPE_FLOAT) ? 4 : 8;
    s->array_vs = s->V;
    if (!s->is_matrix && d.value_type == DML_ELEMENT_TYPE_FLOAT && (flags & DML_FLAG_FLOAT_ARRAY_REF_STRIDE))
        s->array_vs = 8;  // FloatArrayStore.VALUE_SIZE (FloatArrayStore.java:15)
    s->first = first_key;
    s->last = last_key;
    s->rows = rows;
    s->cols = s->is_matrix ? cols : 1;
    s->stride = s->is_matrix ? s->K + (int64_t)s->V * s->cols : s->K + s->array_vs;

    auto fail = [&](hipError_t e, const char* what) {
        dml_store_destroy(s);
        return set_err(DML_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    hipError_t e;
    const size_t nbytes = (size_t)rows * (size_t)s->cols * (size_t)s->V;
    // A small shard's pushes are latency-bound (a few blocks for microseconds): its
    // streams take the high priority, so that on a GPU shared with a large store (LDA's
    // doc-topic totals beside the word-topic rows, LightLDA.scala:238-239) its kernels
    // are dispatched between the large store's reduce blocks instead of queueing
    // behind the whole reduce, which would hold up the caller's next push.
    int prio_lo = 0, prio_hi = 0;
    if ((e = hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi)) != hipSuccess) return fail(e, "stream priorities");
    const int prio = nbytes <= kSmallStoreBytes ? prio_hi : 0;
    auto mkstream = [&](hipStream_t* st) { return hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio); };
    if ((e = mkstream(&s->stream)) != hipSuccess) return fail(e, "stream");
    if ((e = hipMalloc(&s->data, nbytes)) != hipSuccess) return fail(e, "shard alloc");
    if ((e = hipMemsetAsync(s->data, 0, nbytes, s->stream)) != hipSuccess) return fail(e, "shard zero");
    if (s->adagrad) {
        const size_t n = (size_t)rows * (size_t)s->cols;
        if ((e = hipMalloc((void**)&s->alpha, n * 4)) != hipSuccess) return fail(e, "alpha alloc");
        if ((e = hipMalloc((void**)&s->delta, n * 4)) != hipSuccess) return fail(e, "delta alloc");
        if ((e = hipMemsetAsync(s->alpha, 0, n * 4, s->stream)) != hipSuccess) return fail(e, "alpha zero");
        if ((e = hipMemsetAsync(s->delta, 0, n * 4, s->stream)) != hipSuccess) return fail(e, "delta zero");
        s->cand_n = reduce_blocks(d.value_type, rows, s->cols);
        if ((e = hipMalloc((void**)&s->cand, sizeof(DeltaCand) * (size_t)(s->cand_n + kMdParts))) != hipSuccess)
            return fail(e, "cand alloc");
        if ((e = hipMalloc((void**)&s->md, sizeof(MaxDelta))) != hipSuccess) return fail(e, "md alloc");
        if ((e = hipMemsetAsync(s->md, 0, sizeof(MaxDelta), s->stream)) != hipSuccess) return fail(e, "md zero");
    }
    s->slot_bytes = s->is_matrix ? (size_t)rows * kMaxW * sizeof(int32_t) : 0;
    s->ws_bytes = sizeof(Ctrl) + s->slot_bytes + (s->is_matrix ? (size_t)rows * sizeof(uint32_t) : 0);
    if ((e = mkstream(&s->istream)) != hipSuccess) return fail(e, "index stream");
    if ((e = mkstream(&s->cstream)) != hipSuccess) return fail(e, "copy stream");
    for (Workspace& W : s->ws) {
        if ((e = hipMalloc((void**)&W.base, s->ws_bytes)) != hipSuccess) return fail(e, "workspace alloc");
        W.ctrl = (Ctrl*)W.base;
        W.slot = (int32_t*)(W.base + sizeof(Ctrl));
        W.rowflag = (uint32_t*)(W.base + sizeof(Ctrl) + s->slot_bytes);
        if ((e = hipHostMalloc((void**)&W.hctrl, sizeof(Ctrl), hipHostMallocDefault)) != hipSuccess) return fail(e, "ctrl");
        if ((e = hipEventCreateWithFlags(&W.idx_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "event");
        if ((e = hipEventCreateWithFlags(&W.done, hipEventDisableTiming)) != hipSuccess) return fail(e, "event");
        if ((e = hipEventCreate(&W.applied)) != hipSuccess) return fail(e, "event");
        if ((e = hipEventCreate(&W.kstart)) != hipSuccess) return fail(e, "event");
    }
    if ((e = hipStreamSynchronize(s->stream)) != hipSuccess) return fail(e, "init sync");
    *out = s;
    return DML_OK;
}

void dml_store_destroy(dml_store* s) {
    if (!s) return;
    {
        Entry in(s);
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        if (s->istream) (void)hipStreamSynchronize(s->istream);
        if (s->cstream) (void)hipStreamSynchronize(s->cstream);
        for (auto& p : s->ev_used) {
            bool ring = false;
            for (const Workspace& W : s->ws) ring |= p.first == W.kstart;
            if (!ring) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        }
        for (auto& p : s->ev_free) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
        for (Workspace& W : s->ws) {
            (void)hipFree(W.base);
            (void)hipFree(W.sp);
            if (W.hsp) (void)hipHostFree(W.hsp);
            if (W.hidx) (void)hipHostFree(W.hidx);
            if (W.listed) (void)hipFree(W.listed);
            if (W.hctrl) (void)hipHostFree(W.hctrl);
            if (W.idx_done) (void)hipEventDestroy(W.idx_done);
            if (W.done) (void)hipEventDestroy(W.done);
            if (W.applied) (void)hipEventDestroy(W.applied);
            if (W.kstart) (void)hipEventDestroy(W.kstart);
        }
        (void)hipFree(s->data);
        (void)hipFree(s->data_alt);
        (void)hipFree(s->alpha);
        (void)hipFree(s->delta);
        (void)hipFree(s->cand);
        (void)hipFree(s->md);
        s->neg.destroy();
        s->crec.destroy();
        s->fver.destroy();
        (void)hipFree(s->fbad_dev);
        (void)hipFree(s->dstage);
        if (s->hstage) (void)hipHostFree(s->hstage);
        (void)hipFree(s->dscr);
        for (int i = 0; i < 2; ++i) {
            if (s->xbuf[i]) (void)hipHostFree(s->xbuf[i]);
            if (s->xev[i]) (void)hipEventDestroy(s->xev[i]);
        }
        if (s->stream) (void)hipStreamDestroy(s->stream);
        if (s->istream) (void)hipStreamDestroy(s->istream);
        if (s->cstream) (void)hipStreamDestroy(s->cstream);
    }
    delete s;
}

static int push_host(dml_store* s, const uint8_t* const* bufs, const int64_t* lens, int32_t n) {
    if (n < 0 || (n > 0 && (!bufs || !lens))) return set_err(DML_E_INVALID_ARG, "bad push arguments");
    int rc = begin_call(s);
    if (rc) return rc;
    if (int rc = failed(s)) return rc;
    size_t total = 0;
    std::vector<size_t> offs((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] < 0 || (lens[i] > 0 && !bufs[i])) return set_err(DML_E_INVALID_ARG, "bad push buffer");
        offs[(size_t)i] = total;
        total += ((size_t)lens[i] + 255) & ~(size_t)255;
    }
    // Pinned caller buffers (hipHostMalloc / hipHostRegister) DMA straight into HBM;
    // pageable ones are copied into pinned staging push by push, each push's DMA
    // overlapping the CPU copy of the next. All on the index stream (the index
    // reads the bytes first; the apply waits for the index).
    bool all_pinned = true;
    for (int32_t i = 0; i < n && all_pinned; ++i) {
        if (lens[i] == 0) continue;
        hipPointerAttribute_t attr;
        all_pinned = hipPointerGetAttributes(&attr, bufs[i]) == hipSuccess && attr.type == hipMemoryTypeHost;
    }
    (void)hipGetLastError();  // a pageable pointer leaves an error from the attribute query
    rc = ensure_stage(s, total);
    if (rc) return rc;
    for (int32_t i = 0; i < n; ++i) {
        if (lens[i] == 0) continue;
        const uint8_t* src = bufs[i];
        if (!all_pinned) {
            std::memcpy(s->hstage + offs[(size_t)i], bufs[i], (size_t)lens[i]);
            src = s->hstage + offs[(size_t)i];
        }
        HIPCHK(hipMemcpyAsync(s->dstage + offs[(size_t)i], src, (size_t)lens[i], hipMemcpyHostToDevice, s->istream));
    }
    if (all_pinned && (s->flags & DML_FLAG_ASYNC)) HIPCHK(hipStreamSynchronize(s->istream));  // borrowed bytes
    std::vector<const uint8_t*> dptr((size_t)n);
    for (int32_t i = 0; i < n; ++i) dptr[(size_t)i] = s->dstage + offs[(size_t)i];
    rc = run_batch(s, dptr.data(), lens, n);
    if (rc) return rc;
    if (!(s->flags & DML_FLAG_ASYNC)) return retire_all(s);
    return DML_OK;  // async: the caller's bytes are in staging or already DMA'd
}

int dml_store_push_batch(dml_store* s, const uint8_t* const* bufs, const int64_t* lens, int32_t n) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    return push_host(s, bufs, lens, n);
}

int dml_store_push(dml_store* s, const uint8_t* data, int64_t len) { return dml_store_push_batch(s, &data, &len, 1); }

int dml_store_push_batch_device(dml_store* s, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (n < 0 || (n > 0 && (!dev_bufs || !lens))) return set_err(DML_E_INVALID_ARG, "bad push arguments");
    // no retire-all here: run_batch keeps up to kRing-1 chunks in flight
    if (int rc = failed(s)) return rc;
    for (int32_t i = 0; i < n; ++i)
        if (lens[i] < 0 || (lens[i] > 0 && !dev_bufs[i])) return set_err(DML_E_INVALID_ARG, "bad push buffer");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_err(DML_E_INVALID_ARG, kMisalignedPush);
    return run_batch(s, (const uint8_t* const*)dev_bufs, lens, n);
}

int dml_store_flush(dml_store* s) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    return drain(s);
}

int dml_store_push_seq(dml_store* s, uint64_t* seq) {
    if (int rc = check_store(s)) return rc;
    if (!seq) return set_err(DML_E_INVALID_ARG, "null out");
    std::lock_guard<std::mutex> lk(s->mu);
    *seq = s->call_seq;
    return DML_OK;
}

int dml_store_retire(dml_store* s, uint64_t seq) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    while (!s->pend.empty() && s->pend.front().c.seq <= seq)
        if (int rc = retire_one(s)) return rc;
    return DML_OK;
}

int dml_store_stats(dml_store* s, dml_store_counters* out, int32_t reset) {
    if (int rc = check_store(s)) return rc;
    if (!out) return set_err(DML_E_INVALID_ARG, "null out");
    std::lock_guard<std::mutex> lk(s->mu);
    *out = s->st;
    if (reset) s->st = dml_store_counters{};
    return DML_OK;
}

int dml_store_error_state(dml_store* s, int64_t* bad_key, int32_t* bad_col) {
    if (int rc = check_store(s)) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    if (bad_key) *bad_key = s->err_key;
    if (bad_col) *bad_col = s->err_col;
    return s->err;
}

void dml_store_clear_error(dml_store* s) {
    if (!s) return;
    Entry in(s);
    s->err = 0;
    s->err_key = 0;
    s->err_col = -1;
    if (!s->crec.dev && !s->neg.dev && !s->fver.dev) return;
    // chained commits, owner applies and list fetches resume: behind what is queued, every
    // verdict the store has is open again and none is posted
    (void)hipStreamSynchronize(s->stream);
    s->crec.pending = s->neg.pending = s->fver.pending = false;
    (void)s->crec.reopen(s->stream);
    (void)s->neg.reopen(s->stream);
    (void)s->fver.reopen(s->stream);
    (void)hipStreamSynchronize(s->stream);
}

int dml_store_shape(dml_store* s, int64_t* rows, int32_t* cols) {
    if (int rc = check_store(s)) return rc;
    if (rows) *rows = s->rows;
    if (cols) *cols = s->cols;
    return DML_OK;
}

int dml_store_value_type(dml_store* s, int32_t* value_type, int32_t* adagrad) {
    if (int rc = check_store(s)) return rc;
    if (value_type) *value_type = s->desc.value_type;
    if (adagrad) *adagrad = s->adagrad ? 1 : 0;
    return DML_OK;
}

int dml_store_device_ptr(dml_store* s, void** dev_ptr) {
    if (int rc = check_store(s)) return rc;
    if (!dev_ptr) return set_err(DML_E_INVALID_ARG, "null out");
    *dev_ptr = s->data;
    return DML_OK;
}

}  // extern "C"

// dml_prereduce.hip — the ordered pre-reduce of the sharded path (C-ABI dml_reduce_buckets_dense,
// dml_prereduce_*, dml_prectx_*).
//
// A rank's full-range pushes are summed, in push order, into a partial of the whole
// matrix (or, chained, onto a travelling slice) by the store's own kernels, without a
// store: the engine owns only workspaces [Ctrl | slot rows x kMaxW | rowflag rows].
//   dml_reduce_buckets_dense   one synchronous call, any number of pushes
//   dml_prereduce_begin        a handle on a workspace leased from a per-device pool;
//                              its pieces (plain, two-moment, chained) reduce row blocks
//   dml_prereduce_begin_ctx    a handle on a context's ring of three workspaces, with the
//                              store's speculation: dml_prereduce_verify reads the verdict
//   dml_prereduce_end          the call's status; the workspace goes back, clean or not
// Both begins build the handle with prereduce_new and enqueue the index with
// prereduce_begin_tail; what differs is where the workspace comes from and when its slot
// table may be trusted (the `clean` / `kept` rules beside each).
#include "dml_host.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

using namespace dml;

// ---- workspace layout and a call's geometry ----
struct WsView {
    Ctrl* ctrl = nullptr;
    int32_t* slot = nullptr;
    uint32_t* rowflag = nullptr;
};
struct PreGeom {
    dml_desc desc{};
    int64_t first = 0, rows = 0;
    int32_t cols = 0;
    int K = 4, V = 4;
    int64_t stride = 0;
    int device = 0;
};

namespace {

size_t ws_slot_bytes(int64_t rows) { return (size_t)rows * kMaxW * sizeof(int32_t); }
size_t ws_rowflag_bytes(int64_t rows) { return (size_t)rows * sizeof(uint32_t); }
size_t ws_bytes(int64_t rows) { return sizeof(Ctrl) + ws_slot_bytes(rows) + ws_rowflag_bytes(rows); }
WsView ws_carve(uint8_t* base, int64_t rows) {
    return {(Ctrl*)base, (int32_t*)(base + sizeof(Ctrl)), (uint32_t*)(base + sizeof(Ctrl) + ws_slot_bytes(rows))};
}

PreGeom make_geom(const dml_desc& desc, int64_t first, int64_t rows, int32_t cols, int device) {
    PreGeom g;
    g.desc = desc;
    g.first = first;
    g.rows = rows;
    g.cols = cols;
    g.K = desc_key_bytes(desc);
    g.V = desc_value_bytes(desc);
    g.stride = desc_row_stride(desc, cols);
    g.device = device;
    return g;
}

// AdaGrad matrices (ada_ok): only the two-moment and the chained AdaGrad pieces
int desc_refusal(const dml_desc& d, bool ada_ok) {
    if (d.data_type != 1 || !d.dense_column || (d.ada_grad && !(ada_ok && d.value_type == DML_ELEMENT_TYPE_FLOAT)))
        return set_error(DML_E_UNSUPPORTED, ada_ok ? "pre-reduce supports dense-column matrices"
                                                   : "pre-reduce supports dense-column plain matrices");
    if (d.value_type != 0 && d.value_type != 1 && d.value_type != 3) return set_error(DML_E_BAD_DESC, "bad value type");
    return DML_OK;
}

// Pushes [c0, c0 + nb) as the columns of a Batch; false if one is not whole records.
bool fill_batch(Batch& bt, const void* const* bufs, const int64_t* lens, int c0, int nb, int64_t stride,
                int64_t* max_nrec) {
    for (int j = 0; j < nb; ++j) {
        if (lens[c0 + j] % stride) return false;
        bt.base[j] = (const uint8_t*)bufs[c0 + j];
        bt.len[j] = lens[c0 + j];
        bt.nrec[j] = lens[c0 + j] / stride;
        bt.bidx[j] = c0 + j;
        *max_nrec = std::max(*max_nrec, bt.nrec[j]);
    }
    return true;
}

// A finished call's status: the sync's error, else what the index left in the Ctrl.
int end_status(hipError_t e, const Ctrl& h, const char* repeat_msg) {
    if (e != hipSuccess) return set_error(DML_E_HIP, hipGetErrorString(e));
    if (h.cutoff != kNoPos) return set_error(DML_E_KEY_OUT_OF_SHARD, "pre-reduce: key outside the matrix");
    if (h.no_dup == 0u) return set_error(DML_E_UNSUPPORTED, repeat_msg);
    return DML_OK;
}

}  // namespace

// Per-device pool of pre-reduce workspaces (Ctrl + slot table + rowflags).
// hipMalloc/hipFree per step cost ~0.2 ms of host time (hipFree synchronizes
// the device); leases are taken and returned instead, one per in-flight call.
struct WsLease {
    uint8_t* ptr = nullptr;
    size_t bytes = 0;
    bool clean = false;     // slot table all -1 and rowflags 0 (left so by a clearing pre-reduce)
    Ctrl* hctrl = nullptr;  // pinned host copy of the Ctrl (read without touching a stream)
    // the model rows `clean` was established for: a lease serves any model that fits, and
    // a call of another size lays the table and the rowflags out elsewhere (entries a
    // larger, failed call left beyond a smaller call's table are still there)
    int64_t clean_rows = 0;
};
static std::mutex g_ws_mu;
static std::unordered_map<int, std::vector<WsLease>> g_ws_free;

// Per-device pool of maxDelta candidate buffers for the AdaGrad chain pieces
// (dml_prereduce_chain_piece_ada): n candidates plus the finalize's kMdParts of
// scratch, taken and returned like the workspaces.
struct CandBuf {
    DeltaCand* ptr = nullptr;
    int64_t n = 0;
};
static std::unordered_map<int, std::vector<CandBuf>> g_cand_free;

namespace {

// The first pooled entry of `dev` that `fits`, taken out of the pool.
template <typename T, typename Fits>
bool pool_take(std::unordered_map<int, std::vector<T>>& pool, int dev, Fits fits, T* out) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto& v = pool[dev];
    for (size_t i = 0; i < v.size(); ++i)
        if (fits(v[i])) {
            *out = v[i];
            v.erase(v.begin() + (ptrdiff_t)i);
            return true;
        }
    return false;
}

int ws_acquire(int dev, size_t bytes, WsLease* out) {
    if (pool_take(g_ws_free, dev, [&](const WsLease& l) { return l.bytes >= bytes; }, out)) return DML_OK;
    WsLease l;
    hipError_t e = hipMalloc((void**)&l.ptr, bytes);
    if (e == hipSuccess) e = hipHostMalloc((void**)&l.hctrl, sizeof(Ctrl), hipHostMallocDefault);
    if (e != hipSuccess) {
        if (l.ptr) (void)hipFree(l.ptr);
        return set_error(DML_E_HIP, hipGetErrorString(e));
    }
    l.bytes = bytes;
    *out = l;
    return DML_OK;
}

void ws_release(int dev, const WsLease& l) {
    if (!l.ptr) return;
    std::lock_guard<std::mutex> lk(g_ws_mu);
    g_ws_free[dev].push_back(l);
}

int cand_acquire(int dev, int64_t n, CandBuf* out) {
    if (pool_take(g_cand_free, dev, [&](const CandBuf& b) { return b.n >= n; }, out)) return DML_OK;
    CandBuf b;
    HIPCHK(hipMalloc((void**)&b.ptr, sizeof(DeltaCand) * (size_t)(n + kMdParts)));
    b.n = n;
    *out = b;
    return DML_OK;
}

void cand_release(int dev, const std::vector<CandBuf>& bufs) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    for (const CandBuf& b : bufs)
        if (b.ptr) g_cand_free[dev].push_back(b);
}

}  // namespace

extern "C" {

// Stand-alone ordered pre-reduce (multi-GPU): per-device scratch for Ctrl+slots.
int dml_reduce_buckets_dense(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols,
                             const void* const* dev_bufs, const int64_t* lens, int32_t n, void* dev_out, void* stream) {
    if (!desc || !dev_out || rows <= 0 || cols <= 0 || n < 0 || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad reduce arguments");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    if (int rc = desc_refusal(*desc, false)) return rc;
    const int vt = desc->value_type, K = desc_key_bytes(*desc);
    const int64_t stride = desc_row_stride(*desc, cols);
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    WsLease lease;
    if (int rc = ws_acquire(dev, ws_bytes(rows), &lease)) return rc;
    const WsView w = ws_carve(lease.ptr, rows);
    AdaArgs none{};
    int rc = DML_OK;
    for (int c0 = 0; c0 < std::max(n, 1) && rc == DML_OK; c0 += kMaxW) {
        Batch bt{};
        const int nb = std::max(0, std::min(kMaxW, n - c0));
        int64_t max_nrec = 0;
        if (!fill_batch(bt, dev_bufs, lens, c0, nb, stride, &max_nrec)) {
            rc = set_error(DML_E_TRUNCATED, "ragged full-range bucket");
            break;
        }
        hipError_t e = hipMemsetAsync(lease.ptr, 0xFF, sizeof(Ctrl) + ws_slot_bytes(rows), st);
        if (e == hipSuccess) e = hipMemsetAsync(w.rowflag, 0, ws_rowflag_bytes(rows), st);
        if (e == hipSuccess)
            e = launch_index(bt, nb, max_nrec, stride, K, first_key, rows, w.slot, w.rowflag, w.ctrl, kNoPos, st);
        if (e == hipSuccess)
            e = launch_reduce(vt, c0 == 0 ? kPreReduce : kAdd, dev_out, rows, cols, bt, nb, stride, K, w.slot, nullptr,
                              w.ctrl, kNoPos, none, st, nullptr);
        Ctrl h;
        if (e == hipSuccess) e = hipMemcpyAsync(&h, w.ctrl, sizeof h, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        rc = end_status(e, h, "pre-reduce: a bucket repeats a row");
        if (n == 0) break;
    }
    lease.clean = false;  // this path memsets per chunk and does not track cleanliness
    ws_release(dev, lease);
    return rc;
}

}  // extern "C"

// ---- piecewise pre-reduce (multi-GPU pipelining) ----------------------------
struct dml_prereduce : PreGeom {
    Batch bt{};
    int nb = 0;
    uint8_t* ws = nullptr;
    size_t ws_bytes = 0;
    Ctrl* ctrl = nullptr;
    int32_t* slot = nullptr;
    uint32_t* rowflag = nullptr;
    hipStream_t stream = nullptr;
    int64_t rows_done = 0;  // model rows the pieces reduced (all of them: the slot table is clean again)
    Ctrl* hctrl = nullptr;  // the workspace's pinned Ctrl copy (a lease's: DMA'd right behind the index)
    hipEvent_t idx_ev = nullptr;   // begin stream: key index built
    hipEvent_t last_ev = nullptr;  // piece stream: last piece enqueued so far
    hipStream_t last_st = nullptr;
    bool idx_waited = false;
    bool timed = false;
    hipEvent_t done_ev = nullptr;  // completion of the last piece: last_ev, or its timing stop event
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;  // per-piece start/stop of a timed call
    // speculative calls of a pre-reduce context (dml_prereduce_begin_ctx)
    dml_prectx* ctx = nullptr;
    int wi = -1;            // the context's workspace
    bool spec = false;      // identity / kept-column speculation, verified by the pieces
    bool verified = false;  // dml_prereduce_verify ran (the partial is exact)
    int64_t max_nrec = 0;
    struct PieceRec {
        int64_t block, stride, off, ntask;
        void* out;
    };
    std::vector<PieceRec> prec;  // the pieces as launched (a failed verification re-runs them)
    hipEvent_t rerun_ev = nullptr;
    const Ctrl* hidx = nullptr;  // the workspace's Ctrl as the index left it (speculative calls of the flat shape)
    bool chain_checked = false;  // the first chain piece decided about the up-front identity check
    bool slots_unread = false;   // that check ran after the index: the pieces leave the filled slot table as it is
    bool slots_kept = false;     // int32 chain pieces ran: they keep the table for the step's rollback
    std::vector<CandBuf> cands;  // AdaGrad chain pieces: maxDelta candidates (the last is current), back to the pool at _end
};

// Pre-reduce context (dml_prectx_*): the sharded path's pre-reduce with the
// store's speculation. Three workspaces in a ring, like a store's;
// a verified call keeps its slot table, whose permutations the call three later
// may reuse. The partial is reduce-scattered only after dml_prereduce_verify has
// read the pieces' verdict (and re-run them exactly if it failed).
struct PreWs : WsView {
    uint8_t* base = nullptr;
    Ctrl* hctrl = nullptr;          // pinned Ctrl, copied after the pieces (or their re-run)
    Ctrl* hidx = nullptr;           // pinned Ctrl, copied right after the index (k_flat_ident's choice)
    hipEvent_t ctrl_ev = nullptr;   // that copy done
    hipEvent_t free_ev = nullptr;   // the workspace's last call ended (pieces / re-run done)
    bool used = false, clean = false, kept = false;
    bool busy = false;              // a call holds it: begun, not yet ended
    int kept_nb = 0;
    uint64_t perm = 0;              // kept columns holding verified permutations (tally_verified_pushes)
};
struct dml_prectx : PreGeom {
    std::mutex mu;
    PreWs ws[kRing];
    int next = 0;
    hipStream_t xstream = nullptr;  // Ctrl read-back and re-runs
    dml_store_counters st{};
};

// Pre-reduce kernel timing (dml_prereduce_timing(every)): one call in `every`
// gets start/stop events in its pieces' dispatch packets (events in every packet
// cost ~10 us per launch: at config 2's 0.4 ms calls, 4 pieces per call would
// move the step time itself, so bench.py samples 1 in 16 there and every call of
// config 4's 40 ms calls); _end adds their elapsed time to the totals. Events
// come from a pool.
static std::atomic<int32_t> g_pre_timing{0};  // sample one call in g_pre_timing (0 = off)
static std::atomic<int64_t> g_pre_calls{0};
static std::mutex g_pre_mu;
static double g_pre_ms = 0.0;
static int64_t g_pre_launches = 0;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_pre_pool;

// A call's timing pairs, once its last piece is done: their elapsed time into the totals
// (`ok`: the wait for the pieces succeeded), the events back to the pool.
static void timing_drain(dml_prereduce* p, bool ok) {
    if (p->tev.empty()) return;
    double ms = 0.0;
    for (auto& t : p->tev) {
        float v = 0.f;
        if (ok && hipEventElapsedTime(&v, t.first, t.second) == hipSuccess) ms += v;
    }
    std::lock_guard<std::mutex> lk(g_pre_mu);
    if (ok) {
        g_pre_ms += ms;
        g_pre_launches += (int64_t)p->tev.size();
    }
    g_pre_pool.insert(g_pre_pool.end(), p->tev.begin(), p->tev.end());
    p->tev.clear();
}

static void prereduce_free(dml_prereduce* p) {
    if (p->idx_ev) (void)hipEventDestroy(p->idx_ev);
    if (p->last_ev) (void)hipEventDestroy(p->last_ev);
    if (p->rerun_ev) (void)hipEventDestroy(p->rerun_ev);
    delete p;
}

// ---- what the two begins share ----
// The handle of one call: geometry, the pushes as a Batch, the begin stream.
static int prereduce_new(const PreGeom& g, const void* const* dev_bufs, const int64_t* lens, int n, void* stream,
                         dml_prereduce** out) {
    auto* p = new (std::nothrow) dml_prereduce();
    if (!p) return set_error(DML_E_NOMEM, "out of host memory");
    static_cast<PreGeom&>(*p) = g;
    p->stream = (hipStream_t)stream;
    if (!fill_batch(p->bt, dev_bufs, lens, 0, n, p->stride, &p->max_nrec)) {
        delete p;
        return set_error(DML_E_TRUNCATED, "ragged full-range push");
    }
    p->nb = n;
    p->bt.first = g.first;
    *out = p;
    return DML_OK;
}
static void prereduce_bind(dml_prereduce* p, uint8_t* base, const WsView& w, Ctrl* hctrl) {
    p->ws = base;
    p->ctrl = w.ctrl;
    p->slot = w.slot;
    p->rowflag = w.rowflag;
    p->hctrl = hctrl;
}
// Behind the workspace's reset (`e`: its status) on the begin stream: the complete identity
// check where it pays, the key index, a pinned copy of the Ctrl it left (`copy_out`, or
// null), idx_ev; then the call's timing sample is drawn.
static hipError_t prereduce_begin_tail(dml_prereduce* p, hipError_t e, Ctrl* copy_out) {
    hipStream_t st = p->stream;
    // Full-range pushes whose records are rows in order (Java HashMap<Integer> order)
    // skip the key index: every key is checked (k_ident_full) before the pieces,
    // which take slot = row for them. Complete rather than speculative (a speculative
    // call's pieces verify instead): the reduce-scatter reads the partial as soon as a
    // piece is done. Only for slot tables beyond the caches, where the index's slot
    // atomics go to DRAM (config 4 at N > 1: 160 M records, a 640 MB table; world-1
    // group path 40.8 -> 36.7 ms/call): for config 2's 2 MB table the complete check
    // reads as many key lines as the index and lengthens the index stream's chain, which
    // must end before the running pre-reduce does (0.450 -> 0.490 ms/call, measured).
    if (e == hipSuccess && !p->spec && full_range_beyond_caches(p->bt, p->nb, p->rows, kIdentFullMinBytes)) {
        e = launch_ident_full(p->bt, p->nb, p->max_nrec, p->stride, p->K, p->first, p->rows, p->ctrl, st);
        p->bt.ident_ok = 1;
    }
    if (e == hipSuccess)
        e = launch_index(p->bt, p->nb, p->max_nrec, p->stride, p->K, p->first, p->rows, p->slot, p->rowflag, p->ctrl,
                         kNoPos, st);
    if (e == hipSuccess && copy_out) e = hipMemcpyAsync(copy_out, p->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->idx_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(p->idx_ev, st);
    if (e != hipSuccess) return e;
    const int32_t every = g_pre_timing.load(std::memory_order_relaxed);
    p->timed = every > 0 && g_pre_calls.fetch_add(1, std::memory_order_relaxed) % every == 0;
    return hipSuccess;
}
// A begin whose enqueues failed, after its own unwind of the workspace.
static int prereduce_begin_failed(dml_prereduce* p, hipError_t e) {
    prereduce_free(p);
    return set_error(DML_E_HIP, hipGetErrorString(e));
}

// ---- what a piece, the int32 close and a failed speculation's re-run share on the host ----
static RowMap piece_row_map(const dml_prereduce* p, int64_t block, int64_t stride, int64_t off, void* out) {
    RowMap rm;
    rm.block = block;
    rm.stride = stride;
    rm.off = off;
    rm.rows_total = p->rows;
    rm.out = out;
    return rm;
}
// Pieces on another stream (the index ran on a side stream, overlapping the caller's previous
// work): wait for the index on the host, then enqueue the piece straight behind whatever that
// stream runs (no cross-queue barrier). And the handle's completion event, on first use.
static int piece_begin(dml_prereduce* p, hipStream_t st) {
    if (st != p->stream && !p->idx_waited) {
        HIPCHK(hipEventSynchronize(p->idx_ev));
        p->idx_waited = true;
    }
    if (!p->last_ev) HIPCHK(hipEventCreateWithFlags(&p->last_ev, hipEventDisableTiming));
    return DML_OK;
}
// A sampled call's (p->timed) start / stop pair for one launch, from the pool; the handle keeps
// it until dml_prereduce_end has read it.
static int piece_timing_pair(dml_prereduce* p, std::pair<hipEvent_t, hipEvent_t>* t) {
    *t = {nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(g_pre_mu);
        if (!g_pre_pool.empty()) {
            *t = g_pre_pool.back();
            g_pre_pool.pop_back();
        }
    }
    if (!t->first) {
        HIPCHK(hipEventCreate(&t->first));
        HIPCHK(hipEventCreate(&t->second));
    }
    p->tev.push_back(*t);
    return DML_OK;
}
// model rows a piece covered: blocks of row_block task rows at row_off + q*row_stride
static void piece_count_rows(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off, int64_t ntask_rows) {
    for (int64_t t0 = 0; t0 < ntask_rows; t0 += row_block) {
        const int64_t lo = (t0 / row_block) * row_stride + row_off;
        const int64_t hi = std::min(lo + std::min(row_block, ntask_rows - t0), p->rows);
        if (hi > lo) p->rows_done += hi - lo;
    }
}

// Read a context call's verdict once its pieces are done; if speculation failed,
// re-run the call exactly on the context's stream: a fresh slot table, the full
// key index (repeated rows detected), every recorded piece without speculation.
static int prereduce_verify(dml_prereduce* p, int32_t* rerun) {
    if (rerun) *rerun = 0;
    if (!p->ctx || p->verified) return DML_OK;
    dml_prectx* x = p->ctx;
    PreWs& W = x->ws[p->wi];
    HIPCHK(hipStreamWaitEvent(x->xstream, p->done_ev ? p->done_ev : p->idx_ev, 0));
    HIPCHK(hipMemcpyAsync(W.hctrl, W.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, x->xstream));
    HIPCHK(hipEventRecord(W.ctrl_ev, x->xstream));
    HIPCHK(hipEventSynchronize(W.ctrl_ev));
    const Ctrl h = *W.hctrl;
    x->st.chunks += 1;
    if (p->spec && h.spec_ok != 0u) {
        x->st.spec_chunks += 1;
        const uint64_t perm = tally_verified_pushes(h, p->nb, x->st);
        // every row verified: the table's columns are the pushes' permutations
        if (p->rows_done == p->rows) {
            W.kept = true;
            W.kept_nb = p->nb;
            W.perm = perm;
        }
    } else if (p->spec) {
        x->st.spec_chunks += 1;
        x->st.spec_reruns += 1;
        x->st.indexed_pushes += p->nb;
        Batch bt = p->bt;
        bt.spec = 0;
        bt.keeps = 0;
        bt.kept_cols = 0;
        bt.ident_ok = 0;
        bt.prev = nullptr;
        hipStream_t xs = x->xstream;
        HIPCHK(hipMemsetAsync(W.base, 0xFF, sizeof(Ctrl) + ws_slot_bytes(x->rows), xs));
        HIPCHK(hipMemsetAsync(W.rowflag, 0, ws_rowflag_bytes(x->rows), xs));
        HIPCHK(launch_index(bt, p->nb, p->max_nrec, p->stride, p->K, p->first, p->rows, W.slot, W.rowflag, W.ctrl,
                            kNoPos, xs));
        AdaArgs none{};
        for (const auto& pr : p->prec) {
            const RowMap rm = piece_row_map(p, pr.block, pr.stride, pr.off, pr.out);
            HIPCHK(launch_reduce(p->desc.value_type, kPreReduce, pr.out, pr.ntask, p->cols, bt, p->nb, p->stride,
                                 p->K, W.slot, nullptr, W.ctrl, kNoPos, none, xs, nullptr, LaunchEv{}, rm));
        }
        if (!p->rerun_ev) HIPCHK(hipEventCreateWithFlags(&p->rerun_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(p->rerun_ev, xs));
        p->done_ev = p->rerun_ev;  // consumers of the partial (dml_prereduce_stream_wait) wait for the re-run
        HIPCHK(hipMemcpyAsync(W.hctrl, W.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, xs));
        HIPCHK(hipEventRecord(W.ctrl_ev, xs));
        p->bt = bt;
        p->spec = false;
        if (rerun) *rerun = 1;
    } else {
        tally_checked_pushes(h, p->nb, p->bt.ident_ok != 0, x->st);
    }
    p->verified = true;
    return DML_OK;
}

extern "C" {

int dml_prereduce_begin(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols, const void* const* dev_bufs,
                        const int64_t* lens, int32_t n, void* stream, dml_prereduce** out) {
    if (!desc || !out || rows <= 0 || cols <= 0 || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad pre-reduce arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    if (int rc = desc_refusal(*desc, true)) return rc;
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    dml_prereduce* p = nullptr;
    if (int rc = prereduce_new(make_geom(*desc, first_key, rows, cols, device), dev_bufs, lens, n, stream, &p)) return rc;
    WsLease lease;
    if (int rc = ws_acquire(device, ws_bytes(rows), &lease)) {
        delete p;
        return rc;
    }
    p->ws_bytes = lease.bytes;
    prereduce_bind(p, lease.ptr, ws_carve(lease.ptr, rows), lease.hctrl);
    const bool clean = lease.clean && lease.clean_rows == rows;
    // a clean lease needs only its Ctrl reset (see launch_chunk, dml_store.hip)
    hipError_t e = hipMemsetAsync(p->ws, 0xFF, sizeof(Ctrl) + (clean ? 0 : ws_slot_bytes(rows)), p->stream);
    if (e == hipSuccess && !clean) e = hipMemsetAsync(p->rowflag, 0, ws_rowflag_bytes(rows), p->stream);
    // the index alone writes the Ctrl: copied out behind it, so _end reads it without
    // queueing anything behind the caller's later work
    e = prereduce_begin_tail(p, e, p->hctrl);
    if (e != hipSuccess) {
        // the stream may still reference the workspace: drain it before reuse
        (void)hipStreamSynchronize(p->stream);
        ws_release(device, WsLease{p->ws, p->ws_bytes, false, p->hctrl});
        return prereduce_begin_failed(p, e);
    }
    *out = p;
    return DML_OK;
}

int dml_prereduce_moments_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                int64_t ntask_rows, void* dev_out, void* stream) {
    if (!p || !dev_out || row_block <= 0 || ntask_rows < 0) return set_error(DML_E_INVALID_ARG, "bad piece arguments");
    if (p->ctx || p->desc.value_type != DML_ELEMENT_TYPE_FLOAT || p->cols % 4 || p->cols * 4 >= 4096)
        return set_error(DML_E_UNSUPPORTED, "two-moment pieces: f32 rows of whole 16-B vectors under 4 KiB");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = piece_begin(p, st)) return rc;
    const RowMap rm = piece_row_map(p, row_block, row_stride, row_off, dev_out);
    HIPCHK(launch_moments(ntask_rows, p->cols, p->bt, p->nb, p->stride, p->K, p->slot, p->ctrl, rm, st,
                          LaunchEv{nullptr, p->last_ev}));
    p->done_ev = p->last_ev;
    piece_count_rows(p, row_block, row_stride, row_off, ntask_rows);
    p->last_st = st;
    return DML_OK;
}

}  // extern "C"

// One piece of a pre-reduce handle: `mode` kPreReduce (dml_prereduce_piece: sums from
// zero) or kChain (dml_prereduce_chain_piece: sums onto dev_base, a chained
// reduce-scatter step). Row map, stream rule, completion event and timing are shared.
struct AdaPiece {
    const void* base_delta;
    const void* base_marks;
    void* out_delta;
    void* out_marks;
    void* record;  // the slice's travelling MaxDelta
    bool last;     // last piece of this rank's step over the slice
};
static int prereduce_piece(dml_prereduce* p, int mode, int64_t row_block, int64_t row_stride, int64_t row_off,
                           int64_t ntask_rows, const void* dev_base, void* dev_out, void* stream,
                           const AdaPiece* ap = nullptr, const void* dev_record = nullptr) {
    hipStream_t st = (hipStream_t)stream;  // as given: 0 is HIP's null stream
    if (mode == kChain && !p->chain_checked) {
        // Ascending full-range pushes of a flat shape (config 4's case): verify every
        // key up front (k_ident_full), behind the index on its stream, so the pieces
        // take slot = row and, once the host has seen the verdict, k_flat_ident.
        // Complete, not speculative: a chained slice leaves the rank when its piece
        // ends. (dml_prereduce_begin does this itself for slot tables beyond the
        // caches; the table the index filled is then not read, so it is not clean.)
        p->chain_checked = true;
        if (!p->bt.ident_ok && use_flat(p->desc.value_type, kChain, p->cols, p->bt, p->nb, p->rows) &&
            all_full_range(p->bt, p->nb, p->rows)) {
            HIPCHK(launch_ident_full(p->bt, p->nb, p->rows, p->stride, p->K, p->first, p->rows, p->ctrl, p->stream));
            p->bt.ident_ok = 1;
            p->slots_unread = true;
            HIPCHK(hipMemcpyAsync(p->hctrl, p->ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, p->stream));
            HIPCHK(hipEventRecord(p->idx_ev, p->stream));
            p->idx_waited = false;
        }
        if (p->bt.ident_ok) p->hidx = p->hctrl;  // the verdict k_flat_ident is chosen from
    }
    if (int rc = piece_begin(p, st)) return rc;
    RowMap rm = piece_row_map(p, row_block, row_stride, row_off, dev_out);
    rm.base = dev_base;
    rm.rec = dev_record;
    if (mode == kChainCheckI32) p->slots_kept = true;
    AdaArgs none{};
    // the piece's completion event rides in its dispatch packet (no marker packet between pieces)
    LaunchEv ev{nullptr, p->last_ev};
    if (ap) ev.stop = nullptr;  // the candidates' finalize follows the kernel: last_ev is recorded behind it
    if (p->timed) {  // both timing events ride in the packet too
        std::pair<hipEvent_t, hipEvent_t> t;
        if (int rc = piece_timing_pair(p, &t)) return rc;
        ev = LaunchEv{t.first, t.second};
    }
    // all-identity calls (seen in the index's Ctrl, once the host has waited for it):
    // the lean kernel, when no wave's rows straddle two row blocks of the map
    const int Rw = flat_ident_rows_per_wave(p->desc.value_type, p->cols);
    if (ap) {
        // the vector stream needs no whole waves per row block (its row map is per vector)
        const bool ident = p->hidx && p->idx_waited && flat_ident_ok(*p->hidx, p->bt, p->nb, p->rows, kNoPos);
        const int64_t need = std::max<int64_t>(1, chain_ada_blocks(ident, ntask_rows, p->cols));
        if (p->cands.empty() || p->cands.back().n < need) {
            CandBuf cb;
            if (int rc = cand_acquire(p->device, need, &cb)) return rc;
            p->cands.push_back(cb);
        }
        ChainAda ca{(const float*)ap->base_delta, (float*)ap->out_delta, (const uint32_t*)ap->base_marks,
                    (uint32_t*)ap->out_marks, p->cands.back().ptr};
        int64_t ncand = 0;
        HIPCHK(launch_chain_ada(ident, ntask_rows, p->cols, p->bt, p->nb, p->stride, p->K, p->slot, p->ctrl, rm, ca, st,
                                &ncand, ev));
        // this piece's candidates into the record's pending one; the step's last piece applies
        // the strict > against the earlier ranks once (ties inside the rank: earlier position)
        HIPCHK(launch_maxdelta_finalize(ca.cand, ncand, (MaxDelta*)ap->record, p->bt, p->nb, p->stride, p->K, p->V, st,
                                        ap->last ? kMdApply : kMdDefer));
        HIPCHK(hipEventRecord(p->last_ev, st));
        ev.stop = p->last_ev;
    } else if (p->hidx && p->idx_waited && (row_block % Rw == 0 || ntask_rows <= row_block) &&
        flat_ident_ok(*p->hidx, p->bt, p->nb, p->rows, kNoPos)) {
        if (p->ctx) {
            std::lock_guard<std::mutex> lk(p->ctx->mu);
            p->ctx->st.ident_launches += 1;
        }
        HIPCHK(launch_flat_ident(p->desc.value_type, mode, dev_out, ntask_rows, p->cols, p->bt, p->nb, p->stride,
                                 p->K, p->ctrl, st, nullptr, ev, rm));
    } else
        HIPCHK(launch_reduce(p->desc.value_type, mode, dev_out, ntask_rows, p->cols, p->bt, p->nb, p->stride,
                             p->K, p->slot, nullptr, p->ctrl, kNoPos, none, st, nullptr, ev, rm));
    p->done_ev = ev.stop;
    if (mode == kPreReduce) p->prec.push_back({row_block, row_stride, row_off, ntask_rows, dev_out});
    piece_count_rows(p, row_block, row_stride, row_off, ntask_rows);
    p->last_st = st;
    return DML_OK;
}

extern "C" {

int dml_prereduce_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off, int64_t ntask_rows,
                        void* dev_out, void* stream) {
    if (!p || !dev_out || row_block <= 0 || ntask_rows < 0) return set_error(DML_E_INVALID_ARG, "bad piece arguments");
    if (p->desc.ada_grad) return set_error(DML_E_UNSUPPORTED, "AdaGrad pre-reduce: dml_prereduce_moments_piece");
    return prereduce_piece(p, kPreReduce, row_block, row_stride, row_off, ntask_rows, nullptr, dev_out, stream);
}

int dml_prereduce_chain_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                              int64_t ntask_rows, const void* dev_base, void* dev_out, void* stream) {
    if (!p || !dev_base || !dev_out || row_block <= 0 || ntask_rows < 0)
        return set_error(DML_E_INVALID_ARG, "bad chain piece arguments");
    if (p->desc.ada_grad || (p->desc.value_type != DML_ELEMENT_TYPE_FLOAT && p->desc.value_type != DML_ELEMENT_TYPE_DOUBLE))
        return set_error(DML_E_UNSUPPORTED,
                         "chained pieces: plain fp32 / fp64 matrices (int32 and AdaGrad: dml_group_push_exchange)");
    // what a chain piece writes is forwarded at once: a speculative handle's verdict
    // (dml_prereduce_verify) would come after the slice has left the rank
    if (p->ctx) return set_error(DML_E_UNSUPPORTED, "chained pieces need dml_prereduce_begin (no speculative context)");
    return prereduce_piece(p, kChain, row_block, row_stride, row_off, ntask_rows, dev_base, dev_out, stream);
}

int dml_prereduce_chain_piece_ada(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, const void* base_data, const void* base_delta,
                                  const void* base_marks, void* out_data, void* out_delta, void* out_marks,
                                  void* maxdelta_record, int32_t last_piece, void* stream) {
    if (!p || !base_data || !base_delta || !out_data || !out_delta || !out_marks || !maxdelta_record || row_block <= 0 ||
        ntask_rows < 0)
        return set_error(DML_E_INVALID_ARG, "bad AdaGrad chain piece arguments");
    if (!p->desc.ada_grad || p->desc.value_type != DML_ELEMENT_TYPE_FLOAT)
        return set_error(DML_E_UNSUPPORTED,
                         "AdaGrad chained pieces: a handle begun with the AdaGrad descriptor (plain fp32 / fp64: "
                         "dml_prereduce_chain_piece; int32: dml_group_push_exchange)");
    if (p->ctx) return set_error(DML_E_UNSUPPORTED, "chained pieces need dml_prereduce_begin (no speculative context)");
    const AdaPiece ap{base_delta, base_marks, out_delta, out_marks, maxdelta_record, last_piece != 0};
    return prereduce_piece(p, kChain, row_block, row_stride, row_off, ntask_rows, base_data, out_data, stream, &ap);
}

static int chain_i32_refusal(const dml_prereduce* p) {
    if (p->desc.ada_grad || p->desc.value_type != DML_ELEMENT_TYPE_INT)
        return set_error(DML_E_UNSUPPORTED,
                         "int32 chained pieces: a dense int32 matrix handle (fp32 / fp64: dml_prereduce_chain_piece; "
                         "AdaGrad: dml_prereduce_chain_piece_ada)");
    // the slice leaves the rank right after the step's close: a speculative handle's
    // verdict (dml_prereduce_verify) would come later
    if (p->ctx) return set_error(DML_E_UNSUPPORTED, "chained pieces need dml_prereduce_begin (no speculative context)");
    return DML_OK;
}

int dml_prereduce_chain_piece_i32(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, const void* dev_base, void* dev_out, const void* dev_record,
                                  void* stream) {
    if (!p || !dev_base || !dev_out || !dev_record || ((uintptr_t)dev_record & 7u) || row_block <= 0 || ntask_rows < 0)
        return set_error(DML_E_INVALID_ARG, "bad int32 chain piece arguments");
    if (int rc = chain_i32_refusal(p)) return rc;
    return prereduce_piece(p, kChainCheckI32, row_block, row_stride, row_off, ntask_rows, dev_base, dev_out, stream,
                           nullptr, dev_record);
}

int dml_prereduce_chain_close_i32(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, void* dev_slice, void* dev_record, int32_t ring_step,
                                  void* stream) {
    if (!p || !dev_slice || !dev_record || ((uintptr_t)dev_record & 7u) || row_block <= 0 || ntask_rows < 0 ||
        ring_step < 0)
        return set_error(DML_E_INVALID_ARG, "bad int32 chain close arguments");
    if (int rc = chain_i32_refusal(p)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = piece_begin(p, st)) return rc;
    const RowMap rm = piece_row_map(p, row_block, row_stride, row_off, dev_slice);
    LaunchEv ev{nullptr, p->last_ev};
    if (p->timed) {
        // two launches under one pair: the start event is recorded ahead of the rollback, not
        // put into a packet as the pieces do; the stop event rides in the verdict's
        std::pair<hipEvent_t, hipEvent_t> t;
        if (int rc = piece_timing_pair(p, &t)) return rc;
        HIPCHK(hipEventRecord(t.first, st));
        ev.stop = t.second;
    }
    // undo, mod 2^32, this rank's adds past the step's first negative (waves leave at
    // once while Ctrl::neg_pos is kNoPos), then the verdict: one launch each per step
    if (ntask_rows > 0 && p->nb > 0)
        HIPCHK(launch_rollback_i32((int32_t*)dev_slice, ntask_rows, p->cols, p->bt, p->nb, p->stride, p->K, p->slot,
                                   nullptr, p->ctrl, kNoPos, st, rm));
    HIPCHK(launch_chain_i32_verdict(p->bt, p->nb, p->stride, p->K, p->ctrl, (ChainI32Rec*)dev_record, ring_step, st, ev));
    p->done_ev = ev.stop;
    p->last_st = st;
    return DML_OK;
}

int dml_prereduce_timing(int32_t every) {
    g_pre_timing.store(every > 0 ? every : 0);
    g_pre_calls.store(0);
    return DML_OK;
}

int dml_prereduce_kernel_time(double* ms, int64_t* launches, int32_t reset) {
    if (!ms || !launches) return set_error(DML_E_INVALID_ARG, "null output");
    std::lock_guard<std::mutex> lk(g_pre_mu);
    *ms = g_pre_ms;
    *launches = g_pre_launches;
    if (reset) {
        g_pre_ms = 0.0;
        g_pre_launches = 0;
    }
    return DML_OK;
}

int dml_prereduce_stream_wait(dml_prereduce* p, void* stream) {
    if (!p || !p->done_ev) return set_error(DML_E_INVALID_ARG, "no piece enqueued yet");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, p->done_ev, 0));
    return DML_OK;
}

int dml_prereduce_verify(dml_prereduce* p, int32_t* rerun) {
    if (!p) return set_error(DML_E_INVALID_ARG, "null pre-reduce");
    if (!p->ctx) {  // a call without a context does not speculate
        if (rerun) *rerun = 0;
        return DML_OK;
    }
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    return prereduce_verify(p, rerun);
}

int dml_prereduce_end(dml_prereduce* p) {
    if (!p) return set_error(DML_E_INVALID_ARG, "null pre-reduce");
    const char* const repeat = "pre-reduce: a push repeats a row";
    if (p->ctx) {
        dml_prectx* x = p->ctx;
        std::lock_guard<std::mutex> lk(x->mu);
        PreWs& W = x->ws[p->wi];
        int rc = prereduce_verify(p, nullptr);
        hipError_t e = rc == DML_OK ? hipEventSynchronize(W.ctrl_ev) : hipErrorUnknown;  // pieces / re-run done
        timing_drain(p, e == hipSuccess);
        if (rc == DML_OK) rc = end_status(e, *W.hctrl, repeat);
        // a kept table stays (not clean); a non-speculative call whose pieces covered every
        // row through the clearing kernel left it clean; anything else is memset next time
        W.clean = !W.kept && !p->spec && rc == DML_OK && p->rows_done == p->rows &&
                  reduce_clears_slots(p->desc.value_type, kPreReduce, p->cols);
        if (rc != DML_OK) W.kept = false;
        (void)hipEventRecord(W.free_ev, x->xstream);
        W.busy = false;
        prereduce_free(p);
        return rc;
    }
    hipError_t e = hipEventSynchronize(p->idx_ev);  // index done, Ctrl copied out
    const Ctrl h = *p->hctrl;
    // the workspace is free once the last piece ran
    if (e == hipSuccess && p->done_ev) e = hipEventSynchronize(p->done_ev);
    timing_drain(p, e == hipSuccess);
    const int rc = end_status(e, h, repeat);
    // after a failed sync the device state is unknown: drop the lease. A normal chunk
    // whose pieces reduced every row through the clearing kernel left the table clean.
    // (a chained call's late identity check: the pushes it confirmed left their indexed
    // slots unread and uncleared; pushes it rejected were read and cleared like any other)
    const uint64_t pushes = p->nb >= 64 ? ~0ull : (1ull << p->nb) - 1ull;
    if (p->slots_unread && !(h.ident & pushes)) p->slots_unread = false;
    const bool clean = rc == DML_OK && !p->slots_unread && !p->slots_kept && p->rows_done == p->rows &&
                       reduce_clears_slots(p->desc.value_type, kPreReduce, p->cols);
    if (e == hipSuccess) ws_release(p->device, WsLease{p->ws, p->ws_bytes, clean, p->hctrl, p->rows});
    if (e == hipSuccess) cand_release(p->device, p->cands);
    prereduce_free(p);
    return rc;
}

int dml_prectx_create(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols, int32_t device,
                      dml_prectx** out) {
    if (!desc || !out || rows <= 0 || cols <= 0) return set_error(DML_E_INVALID_ARG, "bad pre-reduce context arguments");
    *out = nullptr;
    if (int rc = desc_refusal(*desc, false)) return rc;
    if (rows > INT32_MAX) return set_error(DML_E_INVALID_ARG, "matrix larger than a Java array");
    DeviceGuard g(device);
    auto* x = new (std::nothrow) dml_prectx();
    if (!x) return set_error(DML_E_NOMEM, "out of host memory");
    static_cast<PreGeom&>(*x) = make_geom(*desc, first_key, rows, cols, device);
    auto fail = [&](hipError_t e) {
        dml_prectx_destroy(x);
        return set_error(DML_E_HIP, std::string("pre-reduce context: ") + hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&x->xstream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    for (PreWs& W : x->ws) {
        if ((e = hipMalloc((void**)&W.base, ws_bytes(rows))) != hipSuccess) return fail(e);
        static_cast<WsView&>(W) = ws_carve(W.base, rows);
        if ((e = hipHostMalloc((void**)&W.hctrl, sizeof(Ctrl), hipHostMallocDefault)) != hipSuccess) return fail(e);
        if ((e = hipEventCreateWithFlags(&W.ctrl_ev, hipEventDisableTiming)) != hipSuccess) return fail(e);
        if ((e = hipEventCreateWithFlags(&W.free_ev, hipEventDisableTiming)) != hipSuccess) return fail(e);
    }
    *out = x;
    return DML_OK;
}

void dml_prectx_destroy(dml_prectx* x) {
    if (!x) return;
    {
        std::lock_guard<std::mutex> lk(x->mu);
        DeviceGuard g(x->device);
        if (x->xstream) (void)hipStreamSynchronize(x->xstream);
        for (PreWs& W : x->ws) {
            if (W.free_ev) (void)hipEventSynchronize(W.free_ev);
            (void)hipFree(W.base);
            if (W.hidx) (void)hipHostFree(W.hidx);
            if (W.hctrl) (void)hipHostFree(W.hctrl);
            if (W.ctrl_ev) (void)hipEventDestroy(W.ctrl_ev);
            if (W.free_ev) (void)hipEventDestroy(W.free_ev);
        }
        if (x->xstream) (void)hipStreamDestroy(x->xstream);
    }
    delete x;
}

int dml_prectx_stats(dml_prectx* x, dml_store_counters* out, int32_t reset) {
    if (!x || !out) return set_error(DML_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(x->mu);
    *out = x->st;
    if (reset) x->st = dml_store_counters{};
    return DML_OK;
}

int dml_prereduce_begin_ctx(dml_prectx* x, const void* const* dev_bufs, const int64_t* lens, int32_t n, void* stream,
                            dml_prereduce** out) {
    if (!x || !out || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad pre-reduce arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    std::lock_guard<std::mutex> lk(x->mu);
    DeviceGuard g(x->device);
    // the ring's next workspace must have been ended: a call still holding it would
    // have its Ctrl and slot table rewritten under its pieces
    if (x->ws[x->next].busy)
        return set_error(DML_E_INVALID_ARG, "three calls of this pre-reduce context are outstanding: end one first");
    dml_prereduce* p = nullptr;
    if (int rc = prereduce_new(*x, dev_bufs, lens, n, stream, &p)) return rc;
    const int wi = x->next;
    x->next = (x->next + 1) % kRing;
    PreWs& W = x->ws[wi];
    p->ctx = x;
    p->wi = wi;
    prereduce_bind(p, W.base, W, W.hctrl);
    const int vt = x->desc.value_type;
    // full-range pushes of the speculation shapes: identity / kept-column pushes skip
    // the key index and the pieces verify every record (a failure re-runs the call);
    // other shapes: the complete identity check of prereduce_begin_tail
    p->spec = all_full_range(p->bt, n, x->rows) && spec_shape(vt, x->cols);
    p->bt.spec = p->bt.keeps = p->spec ? 1 : 0;
    p->bt.kept_cols = (p->spec && W.kept && slot_stride(W.kept_nb) == slot_stride(n)) ? W.perm : 0;
    hipStream_t st = p->stream;
    hipError_t e = hipSuccess;
    if (W.used) e = hipStreamWaitEvent(st, W.free_ev, 0);  // its last call's pieces / re-run
    const bool slots_ok = W.clean || (W.kept && p->spec);
    if (e == hipSuccess) e = hipMemsetAsync(W.base, 0xFF, sizeof(Ctrl) + (slots_ok ? 0 : ws_slot_bytes(x->rows)), st);
    if (e == hipSuccess && !(W.clean || W.kept)) e = hipMemsetAsync(W.rowflag, 0, ws_rowflag_bytes(x->rows), st);
    W.clean = W.kept = false;
    W.used = true;
    W.busy = true;
    if (e == hipSuccess && p->spec) {
        e = launch_ident_check(p->bt, n, p->stride, p->K, x->first, x->rows, W.slot, W.ctrl, st);
        if (e == hipSuccess && p->bt.kept_cols) e = launch_assign_cols(W.ctrl, n, st);
    }
    // speculative calls of the flat shape: a pinned copy of the Ctrl the index left, so
    // that the pieces (after the host's wait for the index) can run k_flat_ident
    Ctrl* hidx = nullptr;
    if (e == hipSuccess && p->spec && use_flat(vt, kPreReduce, x->cols, p->bt, n, x->rows)) {
        if (!W.hidx) e = hipHostMalloc((void**)&W.hidx, sizeof(Ctrl), hipHostMallocDefault);
        if (e == hipSuccess) {
            W.hidx->cutoff = 0;  // not all-identity unless the copy lands
            p->hidx = hidx = W.hidx;
        }
    }
    e = prereduce_begin_tail(p, e, hidx);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        (void)hipEventRecord(W.free_ev, st);
        W.busy = false;
        return prereduce_begin_failed(p, e);
    }
    *out = p;
    return DML_OK;
}

}  // extern "C"

// dml_group.hip — native multi-GPU shard group over RCCL (C-ABI dml_group_*).
//
// The JNI deployment has no torch.distributed: one PS process per GPU owns
// shard `rank` of KeyRange.linearSplit(world) (KeyRange.java:68-80,
// DMatrix.partition DMatrix.java:53-64) and reduces device-resident full-range
// pushes with the same three steps as distml_amd/group.py:
//   1. ordered pre-reduce of the rank's pushes into a partial of the whole
//      matrix (dml_prereduce_*, k_reduce_rows in pre-reduce mode), in P row
//      slices laid out [rank][row];
//   2. ncclReduceScatter(sum) of the slices on a communication stream, once the
//      call's speculation is verified: full-range pushes whose records are rows in
//      order, or the permutations a call three before listed, skip the key index
//      and the pieces verify every record (dml_prectx); the next call reads the
//      verdict (a failure re-runs the pieces exactly) and then launches this
//      call's reduce-scatter, so it runs on xGMI under the next call's pre-reduce;
//   3. owner apply shard += received on the store's stream.
// Calls are asynchronous and overlap exactly as in group.py: the next call's key
// index runs on a high-priority side stream, two partial / receive buffer sets
// alternate, and a call's key / repeated-row errors surface at the next call or
// at dml_group_flush. The communicator comes from ncclCommInitRankConfig (the
// channel count pinned, kRsChannels) with a unique id the caller distributes (the
// JVM's control plane).
// dml_group_push_chained (plain fp32 / fp64 and AdaGrad matrices) and
// dml_group_push_chained_i32 (dense int32, IntMatrixStore) are the order-exact alternative:
// each shard's slice walks the ring of ranks over ncclSend / ncclRecv and every rank adds its
// own pushes' rows to it in push order. One driver, chain_push, runs the ring
// for all three kinds of slice; what a kind carries and checks is described at ChainKind. One
// documented divergence (AdaGrad: the alpha of an element whose delta comes home NaN,
// DESIGN.md §2); dml_group_push_exchange is the path without it.
// dml_group_pull is the fetch half (WorkerAgent.fetch, WorkerAgent.java:74-122): a collective call
// in which every rank's device key list is split by owner, owners encode the handleFetch records
// on their store's stream behind every earlier call, and counts, keys and records travel as
// grouped ncclSend / ncclRecv.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "dml_host.h"

using namespace dml;

#define GNCCL(x)                                                                                       \
    do {                                                                                               \
        ncclResult_t r_ = (x);                                                                         \
        if (r_ != ncclSuccess) return set_error(DML_E_HIP, std::string(#x) + ": " + ncclGetErrorString(r_)); \
    } while (0)
#define GRC(x)                     \
    do {                           \
        int rc_ = (x);             \
        if (rc_ != DML_OK) return rc_; \
    } while (0)

struct dml_group {
    int rank = 0, world = 1, device = 0, pieces = 4;
    dml_desc desc{};
    int64_t total_rows = 0, step_rows = 0, shard_first = 0, shard_rows = 0;
    int32_t cols = 0;
    size_t vbytes = 4;
    ncclComm_t comm = nullptr;
    ncclDataType_t dtype = ncclFloat32;
    hipStream_t cstream = nullptr;  // pre-reduce pieces
    hipStream_t istream = nullptr;  // key index of the next call (high priority: its own queue)
    hipStream_t rstream = nullptr;  // reduce-scatter
    dml_store* store = nullptr;
    hipStream_t sstream = nullptr;  // the store's stream (owner apply)
    void* partial[2] = {nullptr, nullptr};
    void* recv[2] = {nullptr, nullptr};
    hipEvent_t rs_done[2] = {nullptr, nullptr};
    hipEvent_t applied[2] = {nullptr, nullptr};
    dml_prectx* pctx = nullptr;  // speculative pre-reduce (workspace ring with kept slot tables)
    // calls whose pieces are enqueued but whose partial is not yet reduce-scattered:
    // the reduce-scatter waits for the call's verdict (dml_prereduce_verify)
    struct Call {
        dml_prereduce* h;  // null when the call failed before its pieces were recorded
        int set;           // partial / recv buffer set
        int rc;            // a local failure of the call's pre-reduce (DML_OK otherwise)
    };
    int fail_verify_at = 0;  // fault injection (dml_group_debug_fail_verify): the n-th next verdict fails
    std::deque<Call> pending;
    int k = 0;
    bool plain = true;  // plain-sum dense matrix: the full-range pre-reduce path applies
    // exchange path (dml_group_push_exchange), two buffer sets alternating by call:
    // split output (read by that call's all-to-all), receive buffer (read by the
    // store when the NEXT call hands it over), count buffers
    void* xsend[2] = {nullptr, nullptr};
    void* xrecv[2] = {nullptr, nullptr};
    int64_t xsend_cap[2] = {0, 0}, xrecv_cap[2] = {0, 0};
    hipEvent_t xsent[2] = {nullptr, nullptr};      // rstream: the set's all-to-all finished
    hipEvent_t xconsumed[2] = {nullptr, nullptr};  // store stream: the store's reduce of the set's slices ran
    // store push-call number of the set's slices (dml_store_push_seq): before the
    // set's receive buffer is overwritten, the store retires that call
    // (dml_store_retire), since a retiring chunk may read its pushes again (exact
    // replay of repeated rows, int32 rollback, re-run of a failed speculation)
    uint64_t xseq[2] = {0, 0};
    int64_t* xcnt = nullptr;  // device [2][world * kMaxW]: counts sent / received
    int xk = 0;
    // received slices of the last call, handed to the store by the next call or the flush
    bool xheld = false;
    int xheld_set = 0;
    std::vector<const void*> xptrs;
    std::vector<int64_t> xlens;
    // two-moment AdaGrad path (dml_group_push_moments), two buffer sets by call:
    // [rank][row][Σu | Σu²] partials and the shard's received moments
    void* mpart[2] = {nullptr, nullptr};
    void* mrecv[2] = {nullptr, nullptr};
    hipEvent_t mrs_done[2] = {nullptr, nullptr};
    hipEvent_t mapplied[2] = {nullptr, nullptr};
    std::deque<dml_prereduce*> mpending;  // calls whose index errors are not yet collected
    int mk = 0;
    // chained path (chain_push), allocated on its first call: two buffer sets by call,
    // each two slice buffers the ring steps alternate between (step t sums in place in
    // the one that step t-1 received into, while the other receives); what a slice
    // buffer holds depends on the kind (ChainKind, chain_sub)
    void* cbuf[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    std::vector<hipEvent_t> cev[2];  // per set: [step][sub-chunk] piece done, then [step][sub-chunk] received
    void* cmd = nullptr;             // AdaGrad: the running step's pending maxDelta candidate (a MaxDelta)
    hipEvent_t cready = nullptr;     // store stream: every earlier call's apply is enqueued before it
    std::deque<dml_prereduce*> cpending;  // calls whose index errors are not yet collected
    int ck = 0;
    // int32 chain: a commit's verdict record is on its way to the host; a non-chained
    // call behind it waits for it first (the reference refuses pushes to a closed store)
    bool cverdict = false;
    // collective pull (dml_group_pull), allocated on its first call and grown on demand: the
    // partition's workspace, [keys by owner | perm], the keys the peers ask this shard for,
    // their records (sent), the records received (request-order mode only)
    void* pws = nullptr;
    void* pkeys = nullptr;
    void* prkeys = nullptr;
    void* psend = nullptr;
    void* precv = nullptr;
    int64_t pws_cap = 0, pkeys_cap = 0, prkeys_cap = 0, psend_cap = 0, precv_cap = 0;
    int64_t* pcnt = nullptr;     // device: [the partition's totals world + 1][asked of q world][asked by q world]
    hipEvent_t pstep = nullptr;  // from one of the pull's streams to the next
    hipEvent_t pdone = nullptr;  // the last pull's last kernel or transfer: one pull is in flight
};

namespace {

constexpr int kRsChannels = 128;  // RCCL CTAs (channels) per collective of the group


// The oldest pending call: read its verdict (a failed speculation re-runs its
// pieces exactly), then reduce-scatter its partial on the communication stream
// and apply the received rows on the store's stream; its errors are returned.
//
// Every rank issues the same collectives in the same order whatever happens
// locally: a rank whose call failed here (its verdict, its re-run, a
// HIP error before the pieces) still enters the reduce-scatter, with a zeroed
// partial, and skips only its own apply; the error is returned to its caller.
// The other ranks' shards then hold every rank's sums except that rank's call.
int finish_front(dml_group* g) {
    dml_group::Call c = g->pending.front();
    g->pending.pop_front();
    int rc = c.rc;
    if (rc == DML_OK) {
        rc = dml_prereduce_verify(c.h, nullptr);
        if (rc == DML_OK && g->fail_verify_at > 0 && --g->fail_verify_at == 0)
            rc = set_error(DML_E_HIP, "injected verify failure (dml_group_debug_fail_verify)");
    }
    if (rc == DML_OK) rc = dml_prereduce_stream_wait(c.h, g->rstream);
    const int64_t S = g->step_rows, P = g->pieces, blk = S / P, W = g->world, C = g->cols;
    uint8_t* part = (uint8_t*)g->partial[c.set];
    // one rank: the [rank][row] slices are the shard's rows in order, the
    // reduce-scatter would be a copy; the owner apply reads the partial itself
    uint8_t* rcv = W == 1 ? part : (uint8_t*)g->recv[c.set];
    const int local = rc;
    if (local != DML_OK && W > 1) {
        // contribute zeros: the pieces (or their re-run) are done with the partial first,
        // and the apply of the call two back (store stream) with this set's recv — a call
        // that failed in _begin_ctx skipped the host wait for it
        (void)hipStreamSynchronize(g->cstream);
        if (c.h) (void)dml_prereduce_stream_wait(c.h, g->rstream);
        (void)hipStreamWaitEvent(g->rstream, g->applied[c.set], 0);
        (void)hipMemsetAsync(part, 0, (size_t)(W * S * C) * g->vbytes, g->rstream);
    }
    int crc = DML_OK;  // the collective's own status
    for (int64_t j = 0; j < P && W > 1; ++j) {
        const ncclResult_t r = ncclReduceScatter(part + (size_t)(j * W * blk * C) * g->vbytes,
                                                 rcv + (size_t)(j * blk * C) * g->vbytes, (size_t)(blk * C), g->dtype,
                                                 ncclSum, g->comm, g->rstream);
        if (r != ncclSuccess && crc == DML_OK)
            crc = set_error(DML_E_HIP, std::string("ncclReduceScatter: ") + ncclGetErrorString(r));
    }
    if (local != DML_OK) {
        // the set stays busy until the zero-contribution reduce-scatter has read the
        // partial and written recv: its next use (two calls on) waits on applied[set],
        // which for this call is the scatter itself (there is no apply)
        if (W > 1) {
            (void)hipEventRecord(g->rs_done[c.set], g->rstream);
            (void)hipEventRecord(g->applied[c.set], g->rstream);
        }
        if (c.h) (void)dml_prereduce_end(c.h);
        return local;
    }
    if (crc != DML_OK) {  // no apply: the set is free once the stream is past the scatter
        (void)hipEventRecord(g->applied[c.set], g->rstream);
        (void)dml_prereduce_end(c.h);
        return crc;
    }
    if (rc == DML_OK && hipEventRecord(g->rs_done[c.set], g->rstream) != hipSuccess) rc = set_error(DML_E_HIP, "event");
    if (rc == DML_OK && hipStreamWaitEvent(g->sstream, g->rs_done[c.set], 0) != hipSuccess)
        rc = set_error(DML_E_HIP, "stream wait");
    if (rc == DML_OK) rc = dml_store_apply_dense_device(g->store, rcv, g->shard_rows * C);
    if (rc == DML_OK && hipEventRecord(g->applied[c.set], g->sstream) != hipSuccess) rc = set_error(DML_E_HIP, "event");
    const int r2 = dml_prereduce_end(c.h);  // the call's key / repeated-row errors
    return rc != DML_OK ? rc : r2;
}

int end_pending(dml_group* g, size_t keep) {
    int rc = DML_OK;
    while (g->pending.size() > keep) {
        const int r = finish_front(g);
        if (rc == DML_OK) rc = r;
    }
    return rc;
}

// The index errors (key outside the matrix, repeated row) of the moments / chained
// calls still held, oldest first, down to `keep` of them.
int end_handles(std::deque<dml_prereduce*>& q, size_t keep) {
    int rc = DML_OK;
    while (q.size() > keep) {
        dml_prereduce* p = q.front();
        q.pop_front();
        const int r = dml_prereduce_end(p);
        if (rc == DML_OK) rc = r;
    }
    return rc;
}
int end_moments(dml_group* g, size_t keep) { return end_handles(g->mpending, keep); }
int end_chained(dml_group* g, size_t keep) { return end_handles(g->cpending, keep); }
// The last int32 chained commit's verdict, waited for: a closed record puts the store into
// its error state (DML_E_NEGATIVE_COUNTER) before the caller hands it anything else.
int chain_i32_verdict(dml_group* g) {
    if (!g->cverdict) return DML_OK;
    g->cverdict = false;
    return store_chain_i32_collect(g->store, true);
}

void group_free(dml_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)end_pending(g, 0);
    (void)end_moments(g, 0);
    (void)end_chained(g, 0);
    if (g->pctx) dml_prectx_destroy(g->pctx);
    if (g->cready) (void)hipEventDestroy(g->cready);
    if (g->cmd) (void)hipFree(g->cmd);
    for (int i = 0; i < 2; ++i) {
        for (void* b : g->cbuf[i])
            if (b) (void)hipFree(b);
        for (hipEvent_t e : g->cev[i]) (void)hipEventDestroy(e);
        if (g->mpart[i]) (void)hipFree(g->mpart[i]);
        if (g->mrecv[i]) (void)hipFree(g->mrecv[i]);
        if (g->mrs_done[i]) (void)hipEventDestroy(g->mrs_done[i]);
        if (g->mapplied[i]) (void)hipEventDestroy(g->mapplied[i]);
    }
    if (g->xcnt) (void)hipFree(g->xcnt);
    for (void* b : {g->pws, g->pkeys, g->prkeys, g->psend, g->precv, (void*)g->pcnt})
        if (b) (void)hipFree(b);
    for (hipEvent_t e : {g->pstep, g->pdone})
        if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
        if (g->xsend[i]) (void)hipFree(g->xsend[i]);
        if (g->xrecv[i]) (void)hipFree(g->xrecv[i]);
        if (g->xsent[i]) (void)hipEventDestroy(g->xsent[i]);
        if (g->xconsumed[i]) (void)hipEventDestroy(g->xconsumed[i]);
        if (g->partial[i]) (void)hipFree(g->partial[i]);
        if (g->recv[i]) (void)hipFree(g->recv[i]);
        if (g->rs_done[i]) (void)hipEventDestroy(g->rs_done[i]);
        if (g->applied[i]) (void)hipEventDestroy(g->applied[i]);
    }
    if (g->comm) (void)ncclCommDestroy(g->comm);
    if (g->store) dml_store_destroy(g->store);
    for (hipStream_t s : {g->cstream, g->istream, g->rstream})
        if (s) (void)hipStreamDestroy(s);
    delete g;
}

int group_init(dml_group* g, const uint8_t* unique_id) {
    HIPCHK(hipSetDevice(g->device));
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithFlags(&g->cstream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithPriority(&g->istream, hipStreamNonBlocking, hi));
    // RCCL's stream is high-priority too: a reduce-scatter's blocks are dispatched
    // ahead of the next call's pre-reduce blocks when both wait for CUs
    HIPCHK(hipStreamCreateWithPriority(&g->rstream, hipStreamNonBlocking, hi));
    // linearSplit(world): every rank's slice of the partial is step_rows long
    std::vector<int64_t> f((size_t)g->world), l((size_t)g->world);
    GRC(dml_linear_split(0, g->total_rows - 1, g->world, f.data(), l.data()));
    g->step_rows = l[0] - f[0] + 1;
    g->shard_first = f[(size_t)g->rank];
    g->shard_rows = l[(size_t)g->rank] - f[(size_t)g->rank] + 1;
    if (g->shard_rows <= 0) return set_error(DML_E_UNSUPPORTED, "empty shard (world > rows)");
    GRC(dml_store_create_range(&g->desc, g->shard_first, l[(size_t)g->rank], g->cols, g->device, 0, &g->store));
    void* ss = nullptr;
    GRC(dml_store_stream(g->store, &ss));
    g->sstream = (hipStream_t)ss;
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipEventCreateWithFlags(&g->rs_done[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->applied[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->xsent[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->xconsumed[i], hipEventDisableTiming));
    }
    HIPCHK(hipMalloc((void**)&g->xcnt, sizeof(int64_t) * 4 * (size_t)g->world * kMaxW));
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    // The reduce-scatter's channel count is pinned instead of left to RCCL's tuning: one
    // rank's ring footprint emulated on one GPU beside the real pre-reduce (DESIGN.md §6,
    // bench.py --emulate-rs) runs N = 4 / 8 at 2.6x / 5.3x the one-GPU store with 32
    // blocks, 3.0x / 6.1x with 64 and 3.4x / 6.7x with 128
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.minCTAs = kRsChannels;
    cfg.maxCTAs = kRsChannels;
    GNCCL(ncclCommInitRankConfig(&g->comm, g->world, id, g->rank, &cfg));
    return DML_OK;
}

// Full-range buffers on first use (an exchange-only group never allocates them).
int ensure_partials(dml_group* g) {
    if (g->partial[0]) return DML_OK;
    const size_t part = (size_t)g->world * (size_t)g->step_rows * (size_t)g->cols * g->vbytes;
    const size_t rcv = (size_t)g->step_rows * (size_t)g->cols * g->vbytes;
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipMalloc(&g->partial[i], part));
        if (g->world > 1) HIPCHK(hipMalloc(&g->recv[i], rcv));  // one rank applies the partial itself
    }
    GRC(dml_prectx_create(&g->desc, 0, g->total_rows, g->cols, g->device, &g->pctx));
    return DML_OK;
}

// Hand the last exchange call's received slices to the store, in rank-major push
// order. Its all-to-all must be complete (the caller synchronized rstream).
int hand_over(dml_group* g) {
    if (!g->xheld) return DML_OK;
    g->xheld = false;
    if (g->xptrs.empty()) return DML_OK;
    const int rc = dml_store_push_batch_device(g->store, g->xptrs.data(), g->xlens.data(), (int32_t)g->xptrs.size());
    // the store's device reads of the set are queued on its stream by now (index
    // host-waited, reduce enqueued); its host-side retire may read them once more
    HIPCHK(hipEventRecord(g->xconsumed[g->xheld_set], g->sstream));
    GRC(dml_store_push_seq(g->store, &g->xseq[g->xheld_set]));
    return rc;
}

int grow(void** p, int64_t* cap, int64_t need) {
    if (*cap >= need) return DML_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    const int64_t n = std::max<int64_t>(need, 1) + (need >> 3);  // 12.5 % headroom for the next call
    HIPCHK(hipMalloc(p, (size_t)n));
    *cap = n;
    return DML_OK;
}

}  // namespace

// ---- the chained reduce-scatter: one ring, three kinds of slice -------------------------------
//
// Order-exact chained reduce-scatter (contract: include/distml_ps.h). At ring step t rank r
// holds slice q = (r - t) mod N (the rows of shard q): it adds its pushes' rows of q (a chain
// piece on cstream; step 0 starts from its own shard, later steps sum in place in what arrived
// from r-1), then sends q to r+1 and receives slice q-1 from r-1 (one ncclSend + ncclRecv group
// per sub-chunk on rstream). A slice goes in `pieces` sub-chunks. What step N-1 receives is the
// rank's own slice after every rank's adds: the store commits it on its stream.
// The whole call is enqueued with one host wait, the first piece's for the key index; only then
// is the previous chained call's handle ended (its index errors; its pieces have run by then, or
// are waited for), so the host runs one call ahead of the ring.
// A local failure (first = a code) changes no send and no receive: the rank forwards every slice
// as it holds it.
enum ChainKind {
    // fp32 / fp64 rows. A slice buffer holds the slice's rows; sub-chunk k's transfer runs under
    // sub-chunk k+1's piece (dml_prereduce_chain_piece).
    kChainPlain,
    // AdaGrad (dml_prereduce_chain_piece_ada): a slice buffer holds `pieces` message slots, one per
    // sub-chunk (ChainMsg: data, delta, a touched mark per row); the owner computes alpha once at
    // its commit. The slice's maxDelta record arrives with its last sub-chunk, so the earlier
    // sub-chunks' pieces collect their candidates in the group's own record (cmd, kMdDefer); they
    // are copied into the travelling record once it is there, and the last piece applies them
    // (kMdApply): one strict > per rank against the earlier ranks, whichever piece held the
    // rank's best candidate.
    kChainAda,
    // Dense int32 (IntMatrixStore): a slice buffer holds [record 32 B][rows]; sub-chunk 0's message
    // starts at the record, so the verdict is on the rank before any piece of the step runs. A
    // step is P pieces (dml_prereduce_chain_piece_i32, every add checked), then one close over
    // the whole slice (dml_prereduce_chain_close_i32: rollback past the step's first negative,
    // verdict); no sub-chunk leaves the rank before that. The first-negative word of a step is the
    // handle's Ctrl::neg_pos (all ones after dml_prereduce_begin, handed back so by every close).
    kChainI32,
};

// An AdaGrad sub-chunk of nr rows as it travels, one contiguous message: [data nr x
// cols][delta nr x cols][marks nr x uint32], then, 8-byte aligned, the slice's maxDelta
// record (a whole MaxDelta, DML_MAXDELTA_RECORD_BYTES) on the slice's last sub-chunk.
struct ChainMsg {
    size_t delta, marks, rec, wire;  // byte offsets inside the message; bytes sent
};
static ChainMsg chain_msg(int64_t nr, size_t rowb, bool with_rec) {
    ChainMsg m;
    m.delta = (size_t)nr * rowb;
    m.marks = 2 * m.delta;
    m.rec = (m.marks + (size_t)nr * 4 + 7) & ~(size_t)7;
    m.wire = with_rec ? m.rec + sizeof(MaxDelta) : m.marks + (size_t)nr * 4;
    return m;
}

struct ChainLayout {
    ChainKind kind;
    int P;         // sub-chunks per slice
    size_t rowb;   // bytes of one row of values
    size_t mslot;  // AdaGrad: one message slot, the longest sub-chunk's message (16-byte aligned)
    size_t bytes;  // one slice buffer
};
static ChainLayout chain_layout(ChainKind kind, int64_t step_rows, int P, size_t rowb) {
    ChainLayout L{kind, P, rowb, 0, (size_t)step_rows * rowb};
    if (kind == kChainAda) {
        L.mslot = (chain_msg((step_rows + P - 1) / P, rowb, true).wire + 15) & ~(size_t)15;
        L.bytes = L.mslot * (size_t)P;
    }
    if (kind == kChainI32) L.bytes += sizeof(ChainI32Rec);
    return L;
}

// Sub-chunk k of a slice of `rows` rows: rows [r0, r0 + nr) of the slice (the last may be
// shorter, or empty), where its message and its rows start in a slice buffer, bytes sent.
struct ChainSub {
    int64_t r0, nr;
    size_t msg, data, wire;
    ChainMsg m;  // AdaGrad: the planes inside the message
};
static ChainSub chain_sub(const ChainLayout& L, int64_t rows, int k) {
    ChainSub s{};
    const int64_t per = (rows + L.P - 1) / L.P;
    s.r0 = std::min<int64_t>((int64_t)k * per, rows);
    s.nr = std::min<int64_t>(per, rows - s.r0);
    switch (L.kind) {
        case kChainPlain:
            s.msg = s.data = (size_t)s.r0 * L.rowb;
            s.wire = (size_t)s.nr * L.rowb;
            break;
        case kChainAda:
            s.m = chain_msg(s.nr, L.rowb, k == L.P - 1);
            s.msg = s.data = (size_t)k * L.mslot;
            s.wire = s.m.wire;
            break;
        case kChainI32:  // sub-chunk 0's message starts at the record
            s.data = sizeof(ChainI32Rec) + (size_t)s.r0 * L.rowb;
            s.msg = k == 0 ? 0 : s.data;
            s.wire = (size_t)s.nr * L.rowb + (k == 0 ? sizeof(ChainI32Rec) : 0);
            break;
    }
    return s;
}
// AdaGrad: the slice's maxDelta record sits in its last sub-chunk's slot
static size_t chain_ada_rec(const ChainLayout& L, int64_t rows) {
    const ChainSub s = chain_sub(L, rows, L.P - 1);
    return s.msg + s.m.rec;
}

static int chain_push(dml_group* g, ChainKind kind, const char* refusal, const void* const* dev_bufs,
                      const int64_t* lens, int32_t n) {
    if (!g || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad push arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    // the same answer on every rank, before any send: nobody waits for a peer
    if (refusal) return set_error(DML_E_UNSUPPORTED, refusal);
    const bool ada = kind == kChainAda, i32 = kind == kChainI32;
    HIPCHK(hipSetDevice(g->device));
    int held = DML_OK;
    if (g->xheld) {  // an exchange call's slices come first: the store applies calls in order
        HIPCHK(hipStreamSynchronize(g->rstream));
        held = hand_over(g);
    }
    // Deliberately not alike: fp / AdaGrad return a failed hand-over at once; an int32 store that is
    // closed refuses the slices, which must not keep its rank off the ring: reported as `prior` after it.
    if (!i32) GRC(held);
    const int W = g->world, P = g->pieces;
    if (W == 1) {  // one owner: the store's own ordered (int32: checked) push is the chain
        GRC(held);
        GRC(end_pending(g, 0));
        return dml_store_push_batch_device(g->store, dev_bufs, lens, n);
    }
    // earlier full-range calls: their applies go onto the store's stream now; what they
    // report is returned after this call's ring (the rank never leaves the ring)
    int prior = end_pending(g, 0);
    if (prior == DML_OK) prior = held;
    const int64_t C = g->cols;
    const size_t rowb = (size_t)C * g->vbytes;
    constexpr size_t kRec = sizeof(ChainI32Rec);
    constexpr size_t kRecHead = offsetof(MaxDelta, pend);  // value, row, col
    std::vector<int64_t> f((size_t)W), l((size_t)W);
    GRC(dml_linear_split(0, g->total_rows - 1, W, f.data(), l.data()));
    auto srows = [&](int q) { return l[(size_t)q] - f[(size_t)q] + 1; };
    const ChainLayout L = chain_layout(kind, g->step_rows, P, rowb);
    if (!g->cbuf[0][0]) {  // first chained call: a group that never makes one pays nothing
        for (int i = 0; i < 2; ++i) {
            for (int j = 0; j < 2; ++j) HIPCHK(hipMalloc(&g->cbuf[i][j], L.bytes));
            g->cev[i].resize((size_t)2 * W * P, nullptr);
            for (hipEvent_t& e : g->cev[i]) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        HIPCHK(hipEventCreateWithFlags(&g->cready, hipEventDisableTiming));
        if (ada) HIPCHK(hipMalloc(&g->cmd, sizeof(MaxDelta)));
    }
    const int set = g->ck;
    g->ck ^= 1;
    int first = DML_OK;  // the rank's first local failure of this call
    auto note = [&](int rc) {
        if (rc != DML_OK && first == DML_OK) first = rc;
    };
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) note(set_error(DML_E_HIP, std::string(what) + ": " + hipGetErrorString(e)));
    };
    // the key index of the rank's pushes over the whole model, on the side stream (it
    // overlaps the previous call's tail); a push that is not whole records fails here
    dml_prereduce* h = nullptr;
    note(dml_prereduce_begin(&g->desc, 0, g->total_rows, g->cols, dev_bufs, lens, n, g->istream, &h));
    // the shard as every earlier call leaves it: earlier pushes are retired (the store's
    // value pointer is then current) and cstream waits for what the store's stream holds
    uint64_t seq = 0;
    void* shard = nullptr;
    float* sdelta = nullptr;
    void* srec = nullptr;  // the store's own record: AdaGrad its running maxDelta, int32 its verdict record
    int closed = DML_OK;   // int32 only
    int rs = dml_store_push_seq(g->store, &seq);
    if (rs == DML_OK) rs = dml_store_retire(g->store, seq);
    if (i32) {
        // A store the host knows to be closed (its error state: a negative counter of an earlier
        // push, or a verdict already collected; one that has just come home is looked at without
        // waiting) is no failure of this call: the rank's pushes still go to the other shards; its
        // own slice travels closed.
        if (rs == DML_OK) closed = store_chain_i32_collect(g->store, false);
        if (rs == DML_E_NEGATIVE_COUNTER) {
            closed = rs;
            rs = DML_OK;
        }
        if (closed != DML_OK && closed != DML_E_NEGATIVE_COUNTER) {  // any other store failure: the call's own
            rs = closed;
            closed = DML_OK;
        }
    }
    note(rs);
    GRC(dml_store_device_ptr(g->store, &shard));
    if (ada) GRC(store_adagrad_ptrs(g->store, &sdelta, &srec));
    if (i32) GRC(store_chain_i32_record(g->store, &srec));
    hip(hipEventRecord(g->cready, g->sstream), "hipEventRecord");
    hip(hipStreamWaitEvent(g->cstream, g->cready, 0), "hipStreamWaitEvent");
    uint8_t* const B[2] = {(uint8_t*)g->cbuf[set][0], (uint8_t*)g->cbuf[set][1]};
    hipEvent_t* const pdone = g->cev[set].data();
    hipEvent_t* const rdone = pdone + (size_t)W * P;
    const int nxt = (g->rank + 1) % W, prv = (g->rank + W - 1) % W;
    int crc = DML_OK;  // the transfers' own status
    // step 0's travelling record of the rank's own slice
    if (ada) {  // the store's running maxDelta, with no pending candidate
        uint8_t* const rec = B[0] + chain_ada_rec(L, srows(g->rank));
        hip(hipMemcpyAsync(rec, srec, kRecHead, hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
        hip(hipMemsetAsync(rec + kRecHead, 0, sizeof(MaxDelta) - kRecHead, g->cstream), "hipMemsetAsync");
    }
    if (i32) {
        // the store's device-resident one (a shard an earlier call closed takes no add although
        // the host has not seen that verdict yet), or closed outright
        if (closed != DML_OK) hip(hipMemsetAsync(B[0], 0, kRec, g->cstream), "hipMemsetAsync");
        else hip(hipMemcpyAsync(B[0], srec, kRec, hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
    }
    for (int t = 0; t < W; ++t) {
        const int q = (g->rank - t + W) % W, qin = (q + W - 1) % W;
        const int64_t qrows = srows(q);
        uint8_t* const cur = B[t & 1];       // step t's slice (t > 0: arrived here in step t - 1)
        uint8_t* const in = B[(t + 1) & 1];  // slice qin lands here
        uint8_t* const rec = ada ? cur + chain_ada_rec(L, qrows) : cur;  // the slice's record (plain: none)
        if (ada && P > 1 && first == DML_OK)  // this step's candidates start from none
            hip(hipMemsetAsync(g->cmd, 0, sizeof(MaxDelta), g->cstream), "hipMemsetAsync");
        for (int k = 0; k < P; ++k) {
            const ChainSub s = chain_sub(L, qrows, k);
            const int64_t r0 = s.r0, nr = s.nr;
            const bool lastk = k == P - 1;
            uint8_t* const out = cur + s.data;
            // an empty sub-chunk is still the step's business where the slice's record travels on
            // it (AdaGrad: the last, int32: the first)
            const bool work = nr > 0 || (ada && lastk) || (i32 && k == 0);
            if (work) {
                const uint8_t* const base = t == 0 ? (const uint8_t*)shard + (size_t)r0 * rowb : out;
                if (t > 0) hip(hipStreamWaitEvent(g->cstream, rdone[(t - 1) * P + k], 0), "hipStreamWaitEvent");
                switch (kind) {
                    case kChainPlain:
                        if (first == DML_OK)
                            note(dml_prereduce_chain_piece(h, nr, nr, f[(size_t)q] + r0, nr, base, out, g->cstream));
                        // a failed rank forwards the slice as it holds it (step 0: its own shard's rows)
                        if (first != DML_OK && t == 0)
                            hip(hipMemcpyAsync(out, base, (size_t)nr * rowb, hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
                        break;
                    case kChainAda: {
                        const uint8_t* const bdl = t == 0 ? (const uint8_t*)sdelta + (size_t)r0 * rowb : out + s.m.delta;
                        if (first == DML_OK && lastk && P > 1)
                            hip(hipMemcpyAsync(rec + kRecHead, (const uint8_t*)g->cmd + kRecHead, sizeof(MaxDelta) - kRecHead,
                                               hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
                        // a piece over zero rows (the record's) still names a row block of one
                        if (first == DML_OK)
                            note(dml_prereduce_chain_piece_ada(h, std::max<int64_t>(nr, 1), std::max<int64_t>(nr, 1),
                                                               f[(size_t)q] + r0, nr, base, bdl,
                                                               t == 0 ? nullptr : out + s.m.marks, out, out + s.m.delta,
                                                               out + s.m.marks, lastk ? (void*)rec : g->cmd, lastk ? 1 : 0, g->cstream));
                        // a failed rank forwards the slice as it holds it (step 0: its own shard's planes,
                        // clear marks, the store's record, which is in place already)
                        if (first != DML_OK && t == 0 && nr > 0) {
                            hip(hipMemcpyAsync(out, base, (size_t)nr * rowb, hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
                            hip(hipMemcpyAsync(out + s.m.delta, bdl, (size_t)nr * rowb, hipMemcpyDeviceToDevice, g->cstream),
                                "hipMemcpyAsync");
                            hip(hipMemsetAsync(out + s.m.marks, 0, (size_t)nr * 4, g->cstream), "hipMemsetAsync");
                        }
                        break;
                    }
                    case kChainI32:
                        if (nr <= 0) break;  // only the record: nothing to add
                        if (first == DML_OK)
                            note(dml_prereduce_chain_piece_i32(h, nr, nr, f[(size_t)q] + r0, nr, base, out, cur, g->cstream));
                        // a failed rank forwards the slice as it holds it (step 0: its own shard's rows, the seeded record)
                        if (first != DML_OK && t == 0)
                            hip(hipMemcpyAsync(out, base, (size_t)nr * rowb, hipMemcpyDeviceToDevice, g->cstream), "hipMemcpyAsync");
                        break;
                }
            }
            // Send timing, deliberate. fp / AdaGrad: sub-chunk k goes right behind piece k, under piece
            // k+1 (the overlap `pieces` exists for). int32: nothing leaves the rank before the step's
            // close has the slice's verdict: one event pdone[t] behind the close, then all P sub-chunks.
            if (i32 && !lastk) continue;
            if (i32 && first == DML_OK)
                note(dml_prereduce_chain_close_i32(h, qrows, qrows, f[(size_t)q], qrows, cur + kRec, cur, t, g->cstream));
            const hipEvent_t ready = i32 ? pdone[t] : work ? pdone[t * P + k] : nullptr;
            if (ready) {
                hip(hipEventRecord(ready, g->cstream), "hipEventRecord");
                hip(hipStreamWaitEvent(g->rstream, ready, 0), "hipStreamWaitEvent");
            }
            for (int j = i32 ? 0 : k; j <= k; ++j) {
                // every rank issues this group, empty sub-chunks included (zero bytes)
                const ChainSub so = chain_sub(L, qrows, j), si = chain_sub(L, srows(qin), j);
                ncclResult_t r = ncclGroupStart();
                if (r == ncclSuccess) r = ncclSend(cur + so.msg, so.wire, ncclUint8, nxt, g->comm, g->rstream);
                if (r == ncclSuccess) r = ncclRecv(in + si.msg, si.wire, ncclUint8, prv, g->comm, g->rstream);
                const ncclResult_t re = ncclGroupEnd();
                if (r == ncclSuccess) r = re;
                if (r != ncclSuccess && crc == DML_OK)
                    crc = set_error(DML_E_HIP, std::string("chained ncclSend/ncclRecv: ") + ncclGetErrorString(r));
                hip(hipEventRecord(rdone[t * P + j], g->rstream), "hipEventRecord");
            }
        }
    }
    // home: step N-1 received the rank's own slice (and its record), every rank's adds in it
    hip(hipStreamWaitEvent(g->sstream, rdone[(W - 1) * P + P - 1], 0), "hipStreamWaitEvent");
    const uint8_t* const home = B[W & 1];
    int commit = crc;  // failed transfers: nothing to commit
    if (commit == DML_OK && kind == kChainPlain)
        commit = dml_store_assign_dense_device(g->store, home, g->shard_rows * C);
    for (int k = 0; k < P && commit == DML_OK && ada; ++k) {
        const ChainSub s = chain_sub(L, srows(g->rank), k);
        const uint8_t* const msg = home + s.msg;
        if (s.nr > 0 || k == P - 1)
            commit = store_assign_adagrad(g->store, s.r0, s.nr, msg, msg + s.m.delta, msg + s.m.marks,
                                          k == P - 1 ? msg + s.m.rec : nullptr);
    }
    // int32: a store known closed commits nothing (the slice came home as it left); a verdict is on
    // its way to the host only after a successful commit
    if (commit == DML_OK && i32 && closed == DML_OK) {
        commit = dml_store_assign_dense_i32_device(g->store, home + kRec, g->shard_rows * C, home);
        if (commit == DML_OK) g->cverdict = true;
    }
    if (h) g->cpending.push_back(h);
    const int older = end_chained(g, 1);  // the previous chained call's key / repeated-row errors
    // `closed` last (int32; DML_OK otherwise): it is the store's state, not a failure of this call
    return prior != DML_OK ? prior : first != DML_OK ? first : commit != DML_OK ? commit : older != DML_OK ? older : closed;
}

extern "C" {

int dml_group_unique_id(uint8_t* out, int32_t cap) {
    if (!out || cap < NCCL_UNIQUE_ID_BYTES) return set_error(DML_E_INVALID_ARG, "need 128 bytes for the unique id");
    ncclUniqueId id;
    GNCCL(ncclGetUniqueId(&id));
    memcpy(out, &id, sizeof id);
    return DML_OK;
}

int dml_group_create(const uint8_t* unique_id, int32_t world, int32_t rank, int32_t device, const dml_desc* desc,
                     int64_t total_rows, int32_t cols, int32_t pieces, dml_group** out) {
    if (!unique_id || !desc || !out || world <= 0 || rank < 0 || rank >= world || total_rows <= 0 || cols <= 0 ||
        pieces <= 0)
        return set_error(DML_E_INVALID_ARG, "bad group arguments");
    if (desc->data_type == DML_DATA_TYPE_MATRIX && !desc->dense_column)
        return set_error(DML_E_UNSUPPORTED, "sparse-column matrices are not supported");
    auto* g = new (std::nothrow) dml_group();
    if (!g) return set_error(DML_E_NOMEM, "out of host memory");
    g->world = world;
    g->rank = rank;
    g->device = device;
    g->desc = *desc;
    g->total_rows = total_rows;
    g->cols = cols;
    g->pieces = pieces;
    g->plain = desc->data_type == DML_DATA_TYPE_MATRIX && !desc->ada_grad;
    if (desc->data_type != DML_DATA_TYPE_MATRIX) g->cols = 1;
    switch (desc->value_type) {
        case DML_ELEMENT_TYPE_FLOAT: g->dtype = ncclFloat32; g->vbytes = 4; break;
        case DML_ELEMENT_TYPE_INT: g->dtype = ncclInt32; g->vbytes = 4; break;  // exact: mod 2^32 like the JVM int
        case DML_ELEMENT_TYPE_DOUBLE: g->dtype = ncclFloat64; g->vbytes = 8; break;
        default: delete g; return set_error(DML_E_BAD_DESC, "bad value type");
    }
    if (int rc = group_init(g, unique_id)) {
        group_free(g);
        return rc;
    }
    *out = g;
    return DML_OK;
}

int dml_group_prereduce_stats(dml_group* g, dml_store_counters* out, int32_t reset) {
    if (!g || !out) return set_error(DML_E_INVALID_ARG, "null argument");
    if (!g->pctx) {
        *out = dml_store_counters{};
        return DML_OK;
    }
    return dml_prectx_stats(g->pctx, out, reset);
}

int dml_group_store(dml_group* g, dml_store** store) {
    if (!g || !store) return set_error(DML_E_INVALID_ARG, "null group");
    *store = g->store;
    return DML_OK;
}

int dml_group_push_full_range(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    if (!g || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad push arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    if (!g->plain)
        return set_error(DML_E_UNSUPPORTED, "the full-range pre-reduce path needs a plain-sum matrix (use dml_group_push_exchange)");
    HIPCHK(hipSetDevice(g->device));
    if (g->xheld) {  // an exchange call's slices come first: the store applies calls in order
        HIPCHK(hipStreamSynchronize(g->rstream));
        GRC(hand_over(g));
    }
    GRC(end_chained(g, 0));  // chained calls are committed on the store's stream already: their index errors
    GRC(chain_i32_verdict(g));
    GRC(ensure_partials(g));
    const int64_t S = g->step_rows, P = g->pieces;
    if (S % P) return set_error(DML_E_INVALID_ARG, "pieces must divide the linearSplit step");
    const int64_t blk = S / P, W = g->world, C = g->cols;
    const int k = g->k;
    g->k ^= 1;
    dml_prereduce* h = nullptr;
    int rc = dml_prereduce_begin_ctx(g->pctx, dev_bufs, lens, n, g->istream, &h);
    // buffer set k was used two calls ago: its apply (behind its reduce-scatter) is done
    if (rc == DML_OK && hipEventSynchronize(g->applied[k]) != hipSuccess) rc = set_error(DML_E_HIP, "applied wait");
    uint8_t* part = (uint8_t*)g->partial[k];
    for (int64_t j = 0; j < P && rc == DML_OK; ++j)
        rc = dml_prereduce_piece(h, blk, S, j * blk, W * blk, part + (size_t)(j * W * blk * C) * g->vbytes,
                                 g->cstream);
    if (rc != DML_OK && h) {
        (void)dml_prereduce_end(h);
        h = nullptr;
    }
    // a call that failed here still takes its place in the collective sequence
    // (finish_front contributes zeros for it and reports rc)
    g->pending.push_back({h, k, rc});
    // the previous call: verdict, reduce-scatter (under this call's pieces), apply, errors
    const int r1 = end_pending(g, 1);
    if (rc != DML_OK) {
        const int r2 = end_pending(g, 0);  // this call's failure, reported now
        return r1 != DML_OK ? r1 : r2;
    }
    return r1;
}

int dml_group_push_exchange(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    if (!g || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad push arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    HIPCHK(hipSetDevice(g->device));
    // full-range calls still waiting for their reduce-scatter come first: the store
    // applies calls in order
    GRC(end_pending(g, 0));
    GRC(end_chained(g, 0));
    // an int32 chained call's verdict: the store is in its error state before this call's
    // slices reach it (they are refused at their hand-over). Returned after the
    // exchanges: the rank never leaves them.
    const int verdict = chain_i32_verdict(g);
    const int W = g->world;
    if (W == 1 && verdict != DML_OK) return verdict;
    const int64_t K = desc_key_bytes(g->desc);
    const int64_t stride = g->desc.data_type == DML_DATA_TYPE_MATRIX ? K + (int64_t)g->vbytes * g->cols
                                                                      : K + (int64_t)g->vbytes;
    if (W == 1 && n > 0) {
        // one owner and every key inside the matrix: the split would copy each push whole
        // and nothing crosses a link, so the store takes the pushes themselves (they stay
        // valid until dml_group_flush, the group's contract)
        std::vector<int64_t> cnt((size_t)n);
        GRC(dml_shard_split(&g->desc, g->cols, g->total_rows, 1, dev_bufs, lens, n, nullptr, 0, cnt.data(),
                            g->cstream));
        bool whole = true;
        for (int b = 0; b < n; ++b) whole = whole && cnt[(size_t)b] * stride == lens[b];
        if (whole) {
            if (g->xheld) {  // the previous exchange call's slices come first
                HIPCHK(hipStreamSynchronize(g->rstream));
                GRC(hand_over(g));
            }
            return dml_store_push_batch_device(g->store, dev_bufs, lens, n);
        }
    }
    // Pipelined over calls (two buffer sets): this call's split runs while the
    // previous call's all-to-all moves its slices; the previous slices reach the
    // store once this call's count exchange (queued behind that all-to-all on the
    // same stream) has completed, and the store applies them while this call's
    // all-to-all runs. The only host waits: the split's counts and the count exchange.
    const int i = g->xk;
    g->xk ^= 1;
    int64_t total = 0;
    for (int b = 0; b < n; ++b) total += lens[b];
    HIPCHK(hipEventSynchronize(g->xsent[i]));  // the set's last all-to-all (two calls ago) read xsend[i]
    std::vector<int64_t> cnt((size_t)n * W, 0);  // [push][dest]
    // a local failure (a push that is not whole records, a HIP error) still takes part
    // in both exchanges, sending nothing, so that no peer waits for this rank; the
    // error is returned after them
    int local = grow(&g->xsend[i], &g->xsend_cap[i], total);
    if (local == DML_OK)
        local = dml_shard_split(&g->desc, g->cols, g->total_rows, W, dev_bufs, lens, n, g->xsend[i],
                                g->xsend_cap[i], cnt.data(), g->cstream);
    if (local != DML_OK) std::fill(cnt.begin(), cnt.end(), 0);
    // counts per destination, then per source: mine[d][b] out, theirs[q][b] in (n per peer)
    std::vector<int64_t> mine((size_t)W * n), theirs((size_t)W * n);
    for (int d = 0; d < W; ++d)
        for (int b = 0; b < n; ++b) mine[(size_t)d * n + b] = cnt[(size_t)b * W + d];
    int64_t* dmine = g->xcnt + (size_t)i * 2 * W * kMaxW;
    int64_t* dtheirs = dmine + (size_t)W * kMaxW;
    HIPCHK(hipMemcpyAsync(dmine, mine.data(), sizeof(int64_t) * mine.size(), hipMemcpyHostToDevice, g->rstream));
    GNCCL(ncclGroupStart());
    for (int q = 0; q < W; ++q) {
        GNCCL(ncclSend(dmine + (size_t)q * n, (size_t)n, ncclInt64, q, g->comm, g->rstream));
        GNCCL(ncclRecv(dtheirs + (size_t)q * n, (size_t)n, ncclInt64, q, g->comm, g->rstream));
    }
    GNCCL(ncclGroupEnd());
    HIPCHK(hipMemcpyAsync(theirs.data(), dtheirs, sizeof(int64_t) * theirs.size(), hipMemcpyDeviceToHost, g->rstream));
    HIPCHK(hipStreamSynchronize(g->rstream));  // also completes the previous call's all-to-all
    GRC(hand_over(g));
    std::vector<int64_t> soff((size_t)W + 1, 0), roff((size_t)W + 1, 0);
    for (int q = 0; q < W; ++q) {
        int64_t sb = 0, rb = 0;
        for (int b = 0; b < n; ++b) {
            sb += mine[(size_t)q * n + b] * stride;
            rb += theirs[(size_t)q * n + b] * stride;
        }
        soff[(size_t)q + 1] = soff[(size_t)q] + sb;
        roff[(size_t)q + 1] = roff[(size_t)q] + rb;
    }
    // xrecv[i] was last read by the store for the call two back: its chunks retire
    // (host side) before the buffer is rewritten or freed, its reduce ran before
    // this call's all-to-all writes it (device side)
    GRC(dml_store_retire(g->store, g->xseq[i]));
    if (g->xrecv_cap[i] < roff[(size_t)W]) HIPCHK(hipEventSynchronize(g->xconsumed[i]));
    GRC(grow(&g->xrecv[i], &g->xrecv_cap[i], roff[(size_t)W]));
    HIPCHK(hipStreamWaitEvent(g->rstream, g->xconsumed[i], 0));
    uint8_t* sp = (uint8_t*)g->xsend[i];
    uint8_t* rp = (uint8_t*)g->xrecv[i];
    GNCCL(ncclGroupStart());
    for (int q = 0; q < W; ++q) {
        GNCCL(ncclSend(sp + soff[(size_t)q], (size_t)(soff[(size_t)q + 1] - soff[(size_t)q]), ncclUint8, q, g->comm,
                       g->rstream));
        GNCCL(ncclRecv(rp + roff[(size_t)q], (size_t)(roff[(size_t)q + 1] - roff[(size_t)q]), ncclUint8, q, g->comm,
                       g->rstream));
    }
    GNCCL(ncclGroupEnd());
    HIPCHK(hipEventRecord(g->xsent[i], g->rstream));
    // the owner's pushes, rank-major: rank 0's pushes in order, then rank 1's, ...
    g->xptrs.clear();
    g->xlens.clear();
    int64_t off = 0;
    for (int q = 0; q < W; ++q)
        for (int b = 0; b < n; ++b) {
            const int64_t ln = theirs[(size_t)q * n + b] * stride;
            if (ln > 0) {
                g->xptrs.push_back(rp + off);
                g->xlens.push_back(ln);
            }
            off += ln;
        }
    g->xheld = true;
    g->xheld_set = i;
    return local != DML_OK ? local : verdict;
}

int dml_group_push_moments(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    if (!g || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad push arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    if (!g->desc.ada_grad || g->desc.value_type != DML_ELEMENT_TYPE_FLOAT)
        return set_error(DML_E_UNSUPPORTED, "the two-moment path is for AdaGrad (float) matrices");
    HIPCHK(hipSetDevice(g->device));
    if (g->xheld) {  // earlier calls' slices first: the store applies calls in order
        HIPCHK(hipStreamSynchronize(g->rstream));
        GRC(hand_over(g));
    }
    GRC(end_pending(g, 0));
    const int64_t S = g->step_rows, W = g->world, C = g->cols;
    if (!g->mpart[0]) {
        for (int i = 0; i < 2; ++i) {
            HIPCHK(hipMalloc(&g->mpart[i], (size_t)(W * S * 2 * C) * sizeof(float)));
            HIPCHK(hipMalloc(&g->mrecv[i], (size_t)(S * 2 * C) * sizeof(float)));
            HIPCHK(hipEventCreateWithFlags(&g->mrs_done[i], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&g->mapplied[i], hipEventDisableTiming));
        }
    }
    const int k = g->mk;
    g->mk ^= 1;
    dml_prereduce* h = nullptr;
    int rc = dml_prereduce_begin(&g->desc, 0, g->total_rows, g->cols, dev_bufs, lens, n, g->istream, &h);
    // buffer set k was used two calls ago: its apply (behind its reduce-scatter) is done
    if (rc == DML_OK && hipEventSynchronize(g->mapplied[k]) != hipSuccess) rc = set_error(DML_E_HIP, "applied wait");
    if (rc == DML_OK) rc = dml_prereduce_moments_piece(h, S, S, 0, W * S, g->mpart[k], g->cstream);
    if (rc == DML_OK) rc = dml_prereduce_stream_wait(h, g->rstream);
    const int local = rc;
    if (local != DML_OK) {
        // the same collective on every rank: zeros from this one, no apply here
        (void)hipStreamSynchronize(g->cstream);
        (void)hipEventSynchronize(g->mapplied[k]);
        (void)hipMemsetAsync(g->mpart[k], 0, (size_t)(W * S * 2 * C) * sizeof(float), g->rstream);
    }
    const ncclResult_t r = ncclReduceScatter(g->mpart[k], g->mrecv[k], (size_t)(S * 2 * C), ncclFloat32, ncclSum,
                                             g->comm, g->rstream);
    if (local != DML_OK || r != ncclSuccess) {
        // no apply: the set's next use (two calls on) waits for the scatter instead
        (void)hipEventRecord(g->mapplied[k], g->rstream);
    }
    if (local != DML_OK) {
        if (h) (void)dml_prereduce_end(h);
        return local;
    }
    if (r != ncclSuccess) {
        (void)dml_prereduce_end(h);
        return set_error(DML_E_HIP, std::string("ncclReduceScatter: ") + ncclGetErrorString(r));
    }
    HIPCHK(hipEventRecord(g->mrs_done[k], g->rstream));
    HIPCHK(hipStreamWaitEvent(g->sstream, g->mrs_done[k], 0));
    GRC(dml_store_apply_adagrad_moments_device(g->store, g->mrecv[k], g->shard_rows));
    HIPCHK(hipEventRecord(g->mapplied[k], g->sstream));
    g->mpending.push_back(h);
    return end_moments(g, 1);  // the previous call's errors
}

// Pushes already split to this shard (the reference client's per-partition split,
// SparseMatrix.java:46-60): the store's exact ordered push, after every earlier
// group call, so the store applies calls in the order they were made.
int dml_group_push_local(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    if (!g || n < 0 || n > kMaxW || (n > 0 && (!dev_bufs || !lens)))
        return set_error(DML_E_INVALID_ARG, "bad push arguments (n must be <= 64)");
    if (!push_ptrs_aligned(dev_bufs, n)) return set_error(DML_E_INVALID_ARG, kMisalignedPush);
    HIPCHK(hipSetDevice(g->device));
    if (g->xheld) {  // the last exchange call's slices
        HIPCHK(hipStreamSynchronize(g->rstream));
        GRC(hand_over(g));
    }
    GRC(end_pending(g, 0));  // full-range calls waiting for their reduce-scatter and apply
    GRC(end_chained(g, 0));  // chained calls' commits are on the store's stream already: their index errors
    GRC(chain_i32_verdict(g));
    return dml_store_push_batch_device(g->store, dev_bufs, lens, n);
}

// The chained reduce-scatter's two entry points (contract: include/distml_ps.h): which kind of
// slice the group's matrix travels as, or the refusal; the ring itself is chain_push.
int dml_group_push_chained(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    const bool ada = g && g->desc.data_type == DML_DATA_TYPE_MATRIX && g->desc.ada_grad &&
                     g->desc.value_type == DML_ELEMENT_TYPE_FLOAT;
    const bool refuse = g && ((!g->plain && !ada) || g->desc.value_type == DML_ELEMENT_TYPE_INT);
    return chain_push(g, ada ? kChainAda : kChainPlain,
                      refuse ? "the chained path serves fp32 / fp64 matrices, plain or AdaGrad (int32: use "
                               "dml_group_push_exchange)"
                             : nullptr,
                      dev_bufs, lens, n);
}

int dml_group_push_chained_i32(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n) {
    const bool refuse = g && (!g->plain || !g->desc.dense_column || g->desc.value_type != DML_ELEMENT_TYPE_INT);
    return chain_push(g, kChainI32,
                      refuse ? "dml_group_push_chained_i32 serves dense int32 matrices (fp32 / fp64, plain or AdaGrad: "
                               "dml_group_push_chained)"
                             : nullptr,
                      dev_bufs, lens, n);
}

// The collective group pull (contract: include/distml_ps.h; protocol and ordering argument:
// DESIGN.md §6). WorkerAgent.fetch (WorkerAgent.java:74-122) for key lists in HBM: partition
// the list by owner (cstream), exchange counts and keys (rstream), every owner encodes what it
// was asked for with the store's own k_fetch_vec (the store's stream, behind every earlier
// push), the records come back (rstream) — straight into dev_out in owner-major order, or into
// a receive buffer that k_pull_unsplit permutes into request order.
// A rank that fails locally (bad argument, short cap, a deferred store error) asks for nothing
// or reports late, but makes every send and receive: no peer waits for it. A HIP,
// RCCL or allocation failure in the middle of the protocol is not covered: it returns at once,
// as in dml_group_push_exchange.
int dml_group_pull(dml_group* g, const int64_t* dev_keys, int64_t nkeys, void* dev_out, int64_t cap, int32_t flags,
                   int64_t* out_len, int64_t* out_counts, void* stream) {
    if (!g) return set_error(DML_E_INVALID_ARG, "null group");
    // the same answer on every rank, before any send and before anything is written: nobody waits
    // for a peer (the partition kernels keep one LDS entry per owner)
    if (g->world > DML_PULL_MAX_WORLD)
        return set_error(DML_E_UNSUPPORTED, "dml_group_pull serves groups of at most 64 ranks");
    HIPCHK(hipSetDevice(g->device));
    const int W = g->world, me = g->rank;
    const bool reqorder = (flags & DML_PULL_REQUEST_ORDER) != 0;
    int local = DML_OK;
    if (!out_len || nkeys < 0 || (nkeys > 0 && !dev_keys) || (flags & ~DML_PULL_REQUEST_ORDER))
        local = set_error(DML_E_INVALID_ARG, "bad pull arguments");
    else if (((uintptr_t)dev_keys & 7u) || ((uintptr_t)dev_out & 3u))
        local = set_error(DML_E_INVALID_ARG, "pull keys are 8-byte aligned, the output 4-byte aligned");
    if (out_len) *out_len = 0;
    for (int q = 0; q < W && out_counts; ++q) out_counts[q] = 0;
    if (!g->pdone) {
        HIPCHK(hipMalloc((void**)&g->pcnt, sizeof(int64_t) * (size_t)(3 * W + 1)));
        HIPCHK(hipEventCreateWithFlags(&g->pstep, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&g->pdone, hipEventDisableTiming));
    }
    HIPCHK(hipEventSynchronize(g->pdone));  // the previous pull is done with the buffers below
    // what dml_group_flush drains: the applies and commits of every earlier call are on the
    // store's stream after this, except a held exchange's slices (handed over below)
    int prior = DML_OK;
    auto note = [&](int rc) {
        if (rc != DML_OK && prior == DML_OK) prior = rc;
    };
    note(end_pending(g, 0));
    note(end_moments(g, 0));
    note(end_chained(g, 0));
    note(chain_i32_verdict(g));
    int64_t rec = 0;
    GRC(store_fetch_record_bytes(g->store, &rec));

    // the partition: keys by owner, the counts on the host (the call's first host wait)
    const int64_t n = local == DML_OK ? nkeys : 0;
    std::vector<int64_t> cnt((size_t)W + 1, 0);
    int64_t* pkeys = nullptr;
    int64_t* perm = nullptr;
    if (n > 0) {
        int rc = grow(&g->pws, &g->pws_cap, (int64_t)pull_partition_ws_bytes(n, W));
        if (rc == DML_OK) rc = grow(&g->pkeys, &g->pkeys_cap, 16 * n);
        if (rc == DML_OK) {
            pkeys = (int64_t*)g->pkeys;
            perm = reqorder ? pkeys + n : nullptr;
            HIPCHK(launch_pull_partition(dev_keys, n, g->total_rows, g->step_rows, W, (uint8_t*)g->pws, pkeys, nullptr,
                                         nullptr, perm, g->pcnt, g->cstream));
            HIPCHK(hipMemcpyAsync(cnt.data(), g->pcnt, sizeof(int64_t) * cnt.size(), hipMemcpyDeviceToHost, g->cstream));
            HIPCHK(hipStreamSynchronize(g->cstream));
        }
        if (rc != DML_OK) local = rc;
    }
    int64_t kept = 0;
    for (int q = 0; q < W; ++q) kept += cnt[(size_t)q];
    if (local == DML_OK) {
        *out_len = kept * rec;
        for (int q = 0; q < W && out_counts; ++q) out_counts[q] = cnt[(size_t)q];
        if (kept * rec > cap || (kept > 0 && !dev_out)) local = set_error(DML_E_CAPACITY, "pull output buffer too small");
    }
    if (local != DML_OK) {  // the rank asks for nothing
        std::fill(cnt.begin(), cnt.end(), 0);
        kept = 0;
    }
    std::vector<int64_t> koff((size_t)W + 1, 0);  // owner q's keys / records start at koff[q]
    for (int q = 0; q < W; ++q) koff[(size_t)q + 1] = koff[(size_t)q] + cnt[(size_t)q];
    uint8_t* const out = (uint8_t*)dev_out;
    hipStream_t last = g->sstream;
    int enc = DML_OK;

    if (W == 1) {
        if (g->xheld) {
            HIPCHK(hipStreamSynchronize(g->rstream));
            note(hand_over(g));
        }
        enc = store_pull_encode(g->store, pkeys, kept, out);
    } else {
        // counts: what this rank asks of q goes out, what q asks of this shard comes in
        std::vector<int64_t> theirs((size_t)W, 0);
        int64_t* const dmine = g->pcnt + W + 1;
        int64_t* const dtheirs = dmine + W;
        HIPCHK(hipMemcpyAsync(dmine, cnt.data(), sizeof(int64_t) * (size_t)W, hipMemcpyHostToDevice, g->rstream));
        GNCCL(ncclGroupStart());
        for (int q = 0; q < W; ++q) {
            if (q == me) continue;
            GNCCL(ncclSend(dmine + q, 1, ncclInt64, q, g->comm, g->rstream));
            GNCCL(ncclRecv(dtheirs + q, 1, ncclInt64, q, g->comm, g->rstream));
        }
        GNCCL(ncclGroupEnd());
        HIPCHK(hipMemcpyAsync(theirs.data(), dtheirs, sizeof(int64_t) * (size_t)W, hipMemcpyDeviceToHost, g->rstream));
        HIPCHK(hipStreamSynchronize(g->rstream));  // also completes the previous exchange call's all-to-all
        note(hand_over(g));
        theirs[(size_t)me] = 0;  // the rank's own keys never leave it
        std::vector<int64_t> roff((size_t)W + 1, 0);
        for (int q = 0; q < W; ++q) roff[(size_t)q + 1] = roff[(size_t)q] + theirs[(size_t)q];
        const int64_t nrk = roff[(size_t)W];
        GRC(grow(&g->prkeys, &g->prkeys_cap, nrk * 8));
        GRC(grow(&g->psend, &g->psend_cap, nrk * rec));
        if (reqorder) GRC(grow(&g->precv, &g->precv_cap, kept * rec));
        int64_t* const rkeys = (int64_t*)g->prkeys;
        uint8_t* const sp = (uint8_t*)g->psend;
        uint8_t* const land = reqorder ? (uint8_t*)g->precv : out;  // owner-major either way
        // every rank issues every send and receive, empty ones included (zero elements: they
        // name a valid address all the same)
        auto at = [&](auto* p, int64_t off, int64_t count) { return count > 0 ? (void*)(p + off) : (void*)g->pcnt; };
        // keys
        GNCCL(ncclGroupStart());
        for (int q = 0; q < W; ++q) {
            if (q == me) continue;
            const int64_t ns = cnt[(size_t)q], nr = theirs[(size_t)q];
            GNCCL(ncclSend(at(pkeys, koff[(size_t)q], ns), (size_t)ns, ncclInt64, q, g->comm, g->rstream));
            GNCCL(ncclRecv(at(rkeys, roff[(size_t)q], nr), (size_t)nr, ncclInt64, q, g->comm, g->rstream));
        }
        GNCCL(ncclGroupEnd());
        HIPCHK(hipEventRecord(g->pstep, g->rstream));
        // the encodes, on the store's stream behind every earlier call's apply: the rank's own
        // slice at its owner-major place (it needs no transfer), then one call over the keys of
        // every peer into the packed send buffer
        enc = store_pull_encode(g->store, pkeys + koff[(size_t)me], cnt[(size_t)me], land + koff[(size_t)me] * rec);
        HIPCHK(hipStreamWaitEvent(g->sstream, g->pstep, 0));
        const int enc2 = store_pull_encode(g->store, rkeys, nrk, sp);
        if (enc == DML_OK) enc = enc2;
        HIPCHK(hipEventRecord(g->pstep, g->sstream));
        HIPCHK(hipStreamWaitEvent(g->rstream, g->pstep, 0));
        // records
        GNCCL(ncclGroupStart());
        for (int q = 0; q < W; ++q) {
            if (q == me) continue;
            const int64_t bs = theirs[(size_t)q] * rec, br = cnt[(size_t)q] * rec;
            GNCCL(ncclSend(at(sp, roff[(size_t)q] * rec, bs), (size_t)bs, ncclUint8, q, g->comm, g->rstream));
            GNCCL(ncclRecv(at(land, koff[(size_t)q] * rec, br), (size_t)br, ncclUint8, q, g->comm, g->rstream));
        }
        GNCCL(ncclGroupEnd());
        if (reqorder) HIPCHK(launch_pull_unsplit(land, perm, kept, rec, out, 0, g->rstream));
        last = g->rstream;
    }
    HIPCHK(hipEventRecord(g->pdone, last));
    if (stream) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, g->pdone, 0));
    else HIPCHK(hipEventSynchronize(g->pdone));
    return local != DML_OK ? local : prior != DML_OK ? prior : enc;
}

int dml_group_debug_fail_verify(dml_group* g, int32_t nth) {
    if (!g || nth < 0) return set_error(DML_E_INVALID_ARG, "bad fault-injection arguments");
    g->fail_verify_at = nth;
    return DML_OK;
}

int dml_group_flush(dml_group* g) {
    if (!g) return set_error(DML_E_INVALID_ARG, "null group");
    HIPCHK(hipSetDevice(g->device));
    int rc = DML_OK;
    if (g->xheld) {  // the last exchange call's slices
        rc = hipStreamSynchronize(g->rstream) == hipSuccess ? DML_OK : set_error(DML_E_HIP, "exchange sync");
        if (rc == DML_OK) rc = hand_over(g);
    }
    const int r1 = end_pending(g, 0);
    if (rc == DML_OK) rc = r1;
    const int rm = end_moments(g, 0);
    if (rc == DML_OK) rc = rm;
    const int rch = end_chained(g, 0);
    if (rc == DML_OK) rc = rch;
    const int rcv = chain_i32_verdict(g);
    if (rc == DML_OK) rc = rcv;
    for (hipStream_t s : {g->cstream, g->rstream})
        if (hipStreamSynchronize(s) != hipSuccess && rc == DML_OK) rc = set_error(DML_E_HIP, "group stream sync");
    for (hipEvent_t e : g->applied)
        if (hipEventSynchronize(e) != hipSuccess && rc == DML_OK) rc = set_error(DML_E_HIP, "apply sync");
    const int r2 = dml_store_flush(g->store);
    return rc != DML_OK ? rc : r2;
}

void dml_group_destroy(dml_group* g) { group_free(g); }

}  // extern "C"

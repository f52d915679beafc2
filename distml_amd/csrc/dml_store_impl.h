// dml_store_impl.h — struct dml_store and what its four translation units share. Private to
// them: the group, the pre-reduce engine and the pull go through dml::store_* (dml_internal.h).
//   dml_store.hip        create / destroy, the chunk pipeline, pushes, the error state, dml::set_error
//   dml_store_io.hip     reads and writes of the shard, fetches (dml::store_pull_encode,
//                        store_fetch_record_bytes), checkpoints
//   dml_store_owner.hip  what the group drives on an owner's shard (the other dml::store_* calls)
//   dml_store_diag.hip   rand, synthetic data, knobs, timing, the dml_diag_* floors
#pragma once
#include "dml_host.h"

#include <cstring>
#include <deque>
#include <mutex>
#include <utility>
#include <vector>

namespace dml {
namespace detail __attribute__((visibility("hidden"))) {  // shared by the four files, exported by none

struct Chunk {
    Batch bt{};
    int nb = 0;
    int64_t max_nrec = 0;
    uint64_t tail_cut = kNoPos;
    bool sorted = false;  // array store: partitioned + per-leaf ordered apply (dml_sparse.hip)
    SpPlan sp{};
    SpLayout spl{};
    bool spec = false;     // identity speculation (full-range plain-sum chunk, Batch::spec)
    bool keeps = false;    // speculative chunk: its slot table is kept for the next chunk here (Batch::kept_cols)
    uint64_t seq = 0;      // number of the push call the chunk belongs to (dml_store_push_seq)
    void* in = nullptr;    // matrix shard the chunk reads (the previous chunk's output)
    void* out = nullptr;   // and writes: == in, or the other buffer of a speculative chunk
};

// A sticky verdict in HBM (all bytes 0xFF: open; the kernels that write it close it once) and
// its pinned host copy, DMA'd behind the work that may have closed it and read behind `ev`.
template <typename T>
struct Mirror {
    T* dev = nullptr;
    T* host = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;  // a copy was posted and not read yet
    // Idempotent: the event, the host copy, then the device record, opened on `st`.
    int ensure(hipStream_t st) {
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (!host) HIPCHK(hipHostMalloc((void**)&host, sizeof(T), hipHostMallocDefault));
        if (dev) return DML_OK;
        HIPCHK(hipMalloc((void**)&dev, sizeof(T)));
        return reopen(st);
    }
    // The record as it stands behind everything queued on `st` so far.
    int post(hipStream_t st) {
        HIPCHK(hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(ev, st));
        pending = true;
        return DML_OK;
    }
    // *out = the posted copy, or an open record: none posted, or not landed yet and !block
    int poll(bool block, T* out) {
        memset(out, 0xFF, sizeof(T));
        if (!pending || (!block && hipEventQuery(ev) == hipErrorNotReady)) return DML_OK;
        HIPCHK(hipEventSynchronize(ev));
        pending = false;
        *out = *host;
        return DML_OK;
    }
    int reopen(hipStream_t st) {
        if (dev) HIPCHK(hipMemsetAsync(dev, 0xFF, sizeof(T), st));
        return DML_OK;
    }
    void destroy() {
        (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        if (ev) (void)hipEventDestroy(ev);
    }
};

}  // namespace detail
}  // namespace dml

// One workspace of the pipeline: [Ctrl | slot rows x kMaxW | rowflag rows], in a ring of
// kRing (dml_host.h).
struct Workspace {
    uint8_t* base = nullptr;
    dml::Ctrl* ctrl = nullptr;
    int32_t* slot = nullptr;
    uint32_t* rowflag = nullptr;
    dml::Ctrl* hctrl = nullptr;       // pinned copy of ctrl, written by the chunk's last DMA
    hipEvent_t idx_done = nullptr;    // side stream: index of the chunk built
    hipEvent_t kstart = nullptr;      // main stream: reduce dispatch start (in-packet timestamp)
    hipEvent_t applied = nullptr;     // main stream: chunk applied (in-packet stop of its last kernel)
    hipEvent_t done = nullptr;        // copy stream: ctrl copied out (chunk retired-able)
    uint8_t* sp = nullptr;            // sparse partition buffers (SpLayout), grown on demand
    size_t sp_cap = 0;
    dml::SpStat* hsp = nullptr;       // pinned status of the single-pass sparse partition
    dml::Ctrl* hidx = nullptr;        // pinned copy of ctrl right after the index (flat speculative chunks)
    bool flat_ident = false;          // the chunk's apply runs k_flat_ident (chosen from hidx)
    uint8_t* listed = nullptr;        // rows the chunk's pushes list (Batch::listed), grown on first use
    bool clears = false;              // the chunk's reduce leaves its slot table all -1
    bool clean = false;               // slot table all -1 and rowflags 0: only the Ctrl needs a reset
    // Kept slot table (the last chunk here was a verified speculative chunk): rowflags
    // 0, and column c of [rows][slot_stride(kept_nb)] is the verified permutation of
    // one of that chunk's pushes (indexed or reused, not identity) when bit c of
    // `perm` is set; other columns hold no meaning
    bool kept = false;
    int kept_nb = 0;
    uint64_t perm = 0;
};

struct Pending {
    dml::detail::Chunk c;
    int w = 0;  // workspace index
};

struct dml_store {
    std::mutex mu;
    int device = 0;
    int64_t ident_full_min = dml::kIdentFullMinBytes;  // DML_KNOB_IDENT_FULL_MIN_BYTES
    hipStream_t stream = nullptr;     // applies (reduce / scatter-add), in push order
    hipStream_t istream = nullptr;    // key index of the next chunk, overlapping the current apply
    hipStream_t cstream = nullptr;    // ctrl read-back, off the apply stream
    dml_desc desc{};
    uint32_t flags = 0;
    bool is_matrix = false, adagrad = false;
    int K = 4, V = 4;           // DataDesc keySize / valueSize (DataDesc.java:50-51)
    int array_vs = 4;           // array record value stride
    int64_t first = 0, last = 0, rows = 0;
    int32_t cols = 1;
    int64_t stride = 0;         // record stride
    void* data = nullptr;       // rows*cols values, as of the last retired chunk
    void* data_alt = nullptr;   // second buffer of speculative chunks (allocated on first use)
    float* alpha = nullptr;     // AdaGrad (FloatMatrixStoreAdaGrad.java:23-24)
    float* delta = nullptr;
    dml::DeltaCand* cand = nullptr;
    int64_t cand_n = 0;
    dml::MaxDelta* md = nullptr;
    float initial_alpha = 0.f, min_alpha = 0.f, factor = 1.5f;  // :22, :26
    Workspace ws[dml::kRing];
    size_t slot_bytes = 0, ws_bytes = 0;
    int next_ws = 0;
    uint64_t call_seq = 0;      // push calls accepted so far (dml_store_push_seq)
    dml_store_counters st{};    // pipeline counters (dml_store_stats), counted at retire
    bool no_spec = false;       // DML_FLAG_NO_SPECULATION, or no HBM headroom for data_alt
    std::deque<Pending> pend;   // launched, not yet retired (oldest first), at most kRing-1
    // staging for host-memory pushes
    uint8_t* hstage = nullptr;
    uint8_t* dstage = nullptr;
    size_t stage_cap = 0;
    // fetch / checkpoint transfers: device scratch (encoded records, swapped
    // rows) and two pinned bounce buffers that overlap DMA with the host copy
    uint8_t* dscr = nullptr;
    size_t dscr_cap = 0;
    uint8_t* xbuf[2] = {nullptr, nullptr};
    hipEvent_t xev[2] = {nullptr, nullptr};
    // sticky error (first failure)
    int err = 0;
    int64_t err_key = 0;
    int32_t err_col = -1;
    // The three device verdicts, read by collect_apply_check in this order. Reported, `crec`
    // and `neg` stay closed until dml_store_clear_error; `fver` reopens itself.
    // int32 chained commits (dml_store_assign_dense_i32_device): the closed record they brought home
    dml::detail::Mirror<dml::ChainI32Rec> crec;
    // device fetches (dml_store_fetch_device): the first bad key of the list fetches so far,
    // posted behind every list fetch. fver.ev is recorded behind every device fetch, range form
    // included, and is what the caller's stream waits for.
    dml::detail::Mirror<dml::FetchVerdict> fver;
    unsigned long long* fbad_dev = nullptr;   // lowest bad list index of the running fetch
    int64_t fetch_kernel = 0;                 // DML_KNOB_FETCH_KERNEL
    // int32 owner apply (dml_store_apply_dense_device): index of the first negative final
    // counter, posted behind every checked apply
    dml::detail::Mirror<unsigned long long> neg;
    // timing of the dominant kernel
    const char* kname = nullptr;  // its instantiation, as last launched (dml_store_kernel_name)
    bool timing = false;
    int32_t timing_every = 1;  // time one matrix chunk in timing_every (dml_store_set_timing)
    int64_t timing_k = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
    double timed_ms = 0.0;
    int64_t timed_n = 0;
};

namespace dml {
namespace detail __attribute__((visibility("hidden"))) {

inline int set_err(int code, const std::string& msg) { return set_error(code, msg); }
inline int check_store(const dml_store* s) { return s ? DML_OK : set_err(DML_E_INVALID_ARG, "null store"); }
// The sticky error state as the status of a call that is refused because of it.
inline int failed(const dml_store* s) {
    return s->err ? set_err(s->err, "store is in a failed state (see dml_store_error_state)") : DML_OK;
}
inline int drain(dml_store* s) {  // returns once everything queued on the apply stream is done
    HIPCHK(hipStreamSynchronize(s->stream));
    return DML_OK;
}
inline int vtype_of(const dml_desc& d) { return d.value_type; }
inline int reduce_mode(const dml_store* s) {
    if (s->adagrad) return kAdaGrad;
    if (s->desc.value_type == DML_ELEMENT_TYPE_INT && s->desc.dense_column) return kAddCheckI32;
    return kAdd;
}
inline AdaArgs ada_args(dml_store* s) {
    return AdaArgs{s->alpha, s->delta, s->cand, s->initial_alpha, s->min_alpha, s->factor};
}

// dml_store.hip. begin_call is the entry of every reading / non-push call: all accepted pushes
// applied and checked (read-your-writes). The collect_* read a posted verdict, waiting for it
// with `block` and only once landed without; a closed one becomes the store's first error.
int retire_all(dml_store* s);
int begin_call(dml_store* s);
int collect_chain_check(dml_store* s, bool block);
int collect_fetch_check(dml_store* s, bool block);
int collect_apply_check(dml_store* s, bool block);
int record_error(dml_store* s, int code, int64_t key, int32_t col);
std::pair<hipEvent_t, hipEvent_t> ev_pair(dml_store* s);  // a timing pair, recycled by ev_collect
void ev_collect(dml_store* s);

}  // namespace detail

namespace {  // per translation unit, like DeviceGuard
// What an entry point holds after check_store: the store's lock, on the store's device.
struct Entry {
    std::lock_guard<std::mutex> lk;
    DeviceGuard g;
    explicit Entry(dml_store* s) : lk(s->mu), g(s->device) {}
};
}  // namespace
}  // namespace dml

// dml_store_io.hip — reads and writes of a store's shard: the dense and AdaGrad read-backs,
// fill / setAlpha / maxDelta, handleFetch on the host and on the device (with the owner's side
// of the group pull, dml::store_pull_encode), the big-endian checkpoint calls and the pinned
// host buffers. Every entry begins with begin_call: all accepted pushes applied and checked.
#include "dml_store_impl.h"

#include <algorithm>
#include <cstring>
#include <thread>

using namespace dml;
using namespace dml::detail;

namespace {

// ---- host <-> device transfers for fetch / checkpoint ----------------------
// Pageable destinations go through two pinned bounce buffers: the DMA of chunk
// i+1 runs while the host copies chunk i out (several threads per chunk).
// Pinned destinations (dml_host_alloc, hipHostRegister) are DMA'd directly.
constexpr size_t kXferChunk = 16u << 20;

bool host_pinned(const void* p) {
    hipPointerAttribute_t a;
    const bool pinned = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // a pageable pointer leaves an error from the attribute query
    return pinned;
}

int ensure_scratch(dml_store* s, size_t bytes) {
    if (bytes <= s->dscr_cap) return DML_OK;
    HIPCHK(hipStreamSynchronize(s->stream));  // queued work may still read the old scratch
    if (s->dscr) (void)hipFree(s->dscr);
    s->dscr = nullptr;
    s->dscr_cap = 0;
    HIPCHK(hipMalloc((void**)&s->dscr, bytes));
    s->dscr_cap = bytes;
    return DML_OK;
}

int ensure_xfer(dml_store* s) {
    for (int i = 0; i < 2; ++i) {
        if (!s->xbuf[i]) HIPCHK(hipHostMalloc((void**)&s->xbuf[i], kXferChunk, hipHostMallocDefault));
        if (!s->xev[i]) HIPCHK(hipEventCreateWithFlags(&s->xev[i], hipEventDisableTiming));
    }
    return DML_OK;
}

void host_copy(uint8_t* d, const uint8_t* src, size_t n) {
    constexpr size_t kPart = 2u << 20;
    constexpr size_t kMaxThreads = 4;
    const size_t parts = std::min(kMaxThreads, n / kPart);
    if (parts < 2) {
        std::memcpy(d, src, n);
        return;
    }
    const size_t per = (n / parts + 63) & ~(size_t)63;
    std::thread th[kMaxThreads];
    for (size_t i = 1; i < parts; ++i) {
        const size_t lo = i * per;
        if (lo >= n) break;
        th[i] = std::thread([=] { std::memcpy(d + lo, src + lo, std::min(per, n - lo)); });
    }
    std::memcpy(d, src, std::min(per, n));
    for (size_t i = 1; i < parts; ++i)
        if (th[i].joinable()) th[i].join();
}

// Device -> host after everything queued on s->stream; returns with the bytes in `dst`.
int d2h(dml_store* s, uint8_t* dst, const uint8_t* src, size_t bytes) {
    if (bytes <= (256u << 10) || host_pinned(dst)) {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        return DML_OK;
    }
    if (int rc = ensure_xfer(s)) return rc;
    const size_t n = (bytes + kXferChunk - 1) / kXferChunk;
    auto issue = [&](size_t i) -> hipError_t {
        const size_t off = i * kXferChunk, len = std::min(kXferChunk, bytes - off);
        hipError_t e = hipMemcpyAsync(s->xbuf[i & 1], src + off, len, hipMemcpyDeviceToHost, s->stream);
        return e == hipSuccess ? hipEventRecord(s->xev[i & 1], s->stream) : e;
    };
    HIPCHK(issue(0));
    if (n > 1) HIPCHK(issue(1));
    for (size_t i = 0; i < n; ++i) {
        HIPCHK(hipEventSynchronize(s->xev[i & 1]));
        const size_t off = i * kXferChunk;
        host_copy(dst + off, s->xbuf[i & 1], std::min(kXferChunk, bytes - off));
        if (i + 2 < n) HIPCHK(issue(i + 2));
    }
    return DML_OK;
}

// Host -> device, queued on s->stream; returns once `src` may be reused.
int h2d(dml_store* s, uint8_t* dst, const uint8_t* src, size_t bytes) {
    if (bytes <= (256u << 10) || host_pinned(src)) {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        return DML_OK;
    }
    if (int rc = ensure_xfer(s)) return rc;
    const size_t n = (bytes + kXferChunk - 1) / kXferChunk;
    for (size_t i = 0; i < n; ++i) {
        if (i >= 2) HIPCHK(hipEventSynchronize(s->xev[i & 1]));  // bounce buffer drained by its DMA
        const size_t off = i * kXferChunk, len = std::min(kXferChunk, bytes - off);
        host_copy(s->xbuf[i & 1], src + off, len);
        HIPCHK(hipMemcpyAsync(dst + off, s->xbuf[i & 1], len, hipMemcpyHostToDevice, s->stream));
        HIPCHK(hipEventRecord(s->xev[i & 1], s->stream));
    }
    return drain(s);
}

// The running fetch's lowest bad index, then the sticky verdict (event and host copy first).
int ensure_fetch_record(dml_store* s) {
    if (!s->fbad_dev) {
        HIPCHK(hipMalloc((void**)&s->fbad_dev, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->fbad_dev, 0xFF, sizeof(unsigned long long), s->stream));
    }
    return s->fver.ensure(s->stream);
}

}  // namespace

extern "C" {

int dml_store_read_dense(dml_store* s, void* host_dst, int64_t bytes) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    const int64_t need = s->rows * s->cols * s->V;
    if (!host_dst || bytes < need) return set_err(DML_E_CAPACITY, "destination too small");
    if (int rc = begin_call(s)) return rc;
    HIPCHK(hipMemcpyAsync(host_dst, s->data, (size_t)need, hipMemcpyDeviceToHost, s->stream));
    return drain(s);
}

int dml_store_write_dense(dml_store* s, const void* host_src, int64_t bytes) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    const int64_t need = s->rows * s->cols * s->V;
    if (!host_src || bytes != need) return set_err(DML_E_CAPACITY, "source size does not match the shard");
    if (int rc = begin_call(s)) return rc;
    HIPCHK(hipMemcpyAsync(s->data, host_src, (size_t)need, hipMemcpyHostToDevice, s->stream));
    return drain(s);
}

int dml_store_read_adagrad(dml_store* s, float* alpha_dst, float* delta_dst, int64_t elems) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    if (elems < s->rows * s->cols) return set_err(DML_E_CAPACITY, "destination too small");
    if (int rc = begin_call(s)) return rc;
    const size_t n = (size_t)(s->rows * s->cols) * 4;
    if (alpha_dst) HIPCHK(hipMemcpyAsync(alpha_dst, s->alpha, n, hipMemcpyDeviceToHost, s->stream));
    if (delta_dst) HIPCHK(hipMemcpyAsync(delta_dst, s->delta, n, hipMemcpyDeviceToHost, s->stream));
    return drain(s);
}

int dml_store_read_rows(dml_store* s, int32_t which, int64_t row0, int64_t nrows, void* host_dst, int64_t bytes) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (which < 0 || which > 2 || row0 < 0 || nrows < 0 || row0 > s->rows || nrows > s->rows - row0)
        return set_err(DML_E_INVALID_ARG, "bad row range or array");
    if (which != 0 && !s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    const int64_t esz = which == 0 ? s->V : 4;
    const int64_t need = nrows * s->cols * esz;
    if (need > 0 && (!host_dst || bytes < need)) return set_err(DML_E_CAPACITY, "destination too small");
    if (int rc = begin_call(s)) return rc;
    if (need == 0) return DML_OK;
    const uint8_t* src = (const uint8_t*)(which == 0 ? s->data : which == 1 ? (void*)s->alpha : (void*)s->delta);
    HIPCHK(hipMemcpyAsync(host_dst, src + row0 * s->cols * esz, (size_t)need, hipMemcpyDeviceToHost, s->stream));
    return drain(s);
}

int dml_store_fill(dml_store* s, double v) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    HIPCHK(launch_fill(vtype_of(s->desc), s->data, s->rows * s->cols, v, s->stream));
    return drain(s);
}

int dml_store_set_alpha(dml_store* s, float initial_alpha, float min_alpha, float factor) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    if (int rc = begin_call(s)) return rc;
    // setAlpha: setAlphaValue(initialAlpha) then the three fields (FloatMatrixStoreAdaGrad.java:77-82)
    HIPCHK(launch_fill_f32(s->alpha, s->rows * s->cols, initial_alpha, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->initial_alpha = initial_alpha;
    s->min_alpha = min_alpha;
    s->factor = factor;
    return DML_OK;
}

int dml_store_max_delta(dml_store* s, float* max_delta, int32_t* row, int32_t* col) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    if (int rc = begin_call(s)) return rc;
    MaxDelta m;
    HIPCHK(hipMemcpyAsync(&m, s->md, sizeof m, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    if (max_delta) *max_delta = m.value;
    if (row) *row = m.row;
    if (col) *col = m.col;
    return DML_OK;
}

// Record layout of handleFetch (dense column): bytes per record, and per column in it.
static int64_t fetch_record_bytes(const dml_store* s, int* value_slot) {
    if (s->is_matrix) {
        *value_slot = s->adagrad ? 8 : s->V;
        return s->K + (int64_t)s->cols * *value_slot;
    }
    *value_slot = (s->desc.value_type == DML_ELEMENT_TYPE_FLOAT) ? 8 : s->V;  // FloatArrayStore VALUE_SIZE 8
    return s->K + *value_slot;
}

// keys == nullptr: the keys are key_lo .. key_lo + nkeys - 1 (a KeyRange already
// clipped to the shard), encoded without a key array.
static int fetch_impl(dml_store* s, const int64_t* keys, int64_t nkeys, int64_t key_lo, uint8_t* out, int64_t cap,
                      int64_t* out_len) {
    if (nkeys < 0 || !out_len) return set_err(DML_E_INVALID_ARG, "bad fetch arguments");
    int value_slot;
    const int64_t rec = fetch_record_bytes(s, &value_slot);
    *out_len = nkeys * rec;
    if (!out || cap < *out_len) return set_err(DML_E_CAPACITY, "fetch output buffer too small");
    if (keys) {
        // by range, not by indexOf's narrowed (int)(key - first): the reference intersects a
        // fetch's keys with the shard before any indexOf (FloatMatrixStore.java:116,
        // KeyList.java:74-86), and k_fetch indexes with the 64-bit key - first
        for (int64_t j = 0; j < nkeys; ++j)
            if (keys[j] < s->first || keys[j] > s->last) return record_error(s, DML_E_KEY_OUT_OF_SHARD, keys[j], -1);
    }
    if (nkeys == 0) return DML_OK;
    const size_t kbytes = keys ? ((size_t)nkeys * 8 + 255) & ~(size_t)255 : 0;
    if (int rc = ensure_scratch(s, kbytes + (size_t)*out_len)) return rc;
    const int64_t* dkeys = keys ? (const int64_t*)s->dscr : nullptr;
    if (keys) HIPCHK(hipMemcpyAsync(s->dscr, keys, (size_t)nkeys * 8, hipMemcpyHostToDevice, s->stream));
    uint8_t* dout = s->dscr + kbytes;
    HIPCHK(launch_fetch(vtype_of(s->desc), s->data, s->adagrad ? s->alpha : nullptr, s->cols, dkeys, key_lo, nkeys,
                        s->first, dout, rec, s->K, value_slot, s->stream));
    return d2h(s, out, dout, (size_t)*out_len);
}

int dml_store_fetch(dml_store* s, const int64_t* keys, int64_t nkeys, uint8_t* out, int64_t cap, int64_t* out_len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    if (nkeys > 0 && !keys) return set_err(DML_E_INVALID_ARG, "null keys");
    return fetch_impl(s, keys, nkeys, 0, out, cap, out_len);
}

int dml_store_fetch_range(dml_store* s, int64_t first_key, int64_t last_key, uint8_t* out, int64_t cap,
                          int64_t* out_len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    // KeyRange.intersect (KeyRange.java:124-136): clip to the shard, ascending
    const int64_t lo = std::max(first_key, s->first), hi = std::min(last_key, s->last);
    if (!out_len) return set_err(DML_E_INVALID_ARG, "null out_len");
    return fetch_impl(s, nullptr, lo <= hi ? hi - lo + 1 : 0, lo, out, cap, out_len);
}

// The device fetch behind its entry checks (begin_call done: every accepted push retired, so
// s->data names the shard buffer the last of them wrote). dkeys == nullptr: the range form.
// The encode, the list form's verdict and the event go on the apply stream; the kernels of
// later pushes queue behind them there.
static int fetch_device_impl(dml_store* s, const int64_t* dkeys, int64_t nkeys, int64_t key_lo, void* dev_out,
                             int64_t cap, int64_t* out_len, hipStream_t user) {
    int value_slot;
    const int64_t rec = fetch_record_bytes(s, &value_slot);
    if (((uintptr_t)dev_out & 3) != 0) return set_err(DML_E_INVALID_ARG, "fetch output is not 4-byte aligned");
    if (*out_len > 0 && (!dev_out || cap < *out_len)) return set_err(DML_E_CAPACITY, "fetch output buffer too small");
    if (nkeys == 0) return DML_OK;
    const int which = (int)(s->fetch_kernel & 0xFF), variant = (int)(s->fetch_kernel >> 8);
    if (int rc = ensure_fetch_record(s)) return rc;
    const float* alpha = s->adagrad ? s->alpha : nullptr;
    if (which == 1) {
        if (dkeys)
            HIPCHK(launch_fetch_checked(vtype_of(s->desc), s->data, alpha, s->cols, dkeys, nkeys, s->first, s->last,
                                        (uint8_t*)dev_out, rec, s->K, value_slot, s->fbad_dev, s->stream));
        else
            HIPCHK(launch_fetch(vtype_of(s->desc), s->data, alpha, s->cols, nullptr, key_lo, nkeys, s->first,
                                (uint8_t*)dev_out, rec, s->K, value_slot, s->stream));
    } else {
        // k_fetch_vec takes every dense-column shape and is the dispatch's choice on all of
        // them, so value 2 never meets DML_E_UNSUPPORTED today
        HIPCHK(launch_fetch_vec(vtype_of(s->desc), s->data, alpha, s->cols, dkeys, key_lo, nkeys, s->first, s->last,
                                (uint8_t*)dev_out, rec, s->K, value_slot, s->fbad_dev, variant, s->stream));
    }
    // fver.ev is recorded behind every device fetch, and the caller's stream waits for it; only
    // the list form has a verdict to post in front of it
    if (dkeys) {
        HIPCHK(launch_fetch_verdict(s->fbad_dev, dkeys, s->fver.dev, s->stream));
        if (int rc = s->fver.post(s->stream)) return rc;
    } else {
        HIPCHK(hipEventRecord(s->fver.ev, s->stream));
    }
    if (user) {
        HIPCHK(hipStreamWaitEvent(user, s->fver.ev, 0));
        return DML_OK;
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return collect_fetch_check(s, true);
}

int dml_store_fetch_device(dml_store* s, const int64_t* dev_keys, int64_t nkeys, void* dev_out, int64_t cap,
                           int64_t* out_len, void* stream) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    if (!out_len) return set_err(DML_E_INVALID_ARG, "null out_len");
    if (nkeys < 0) {
        *out_len = 0;
        return set_err(DML_E_INVALID_ARG, "negative key count");
    }
    int slot;
    *out_len = nkeys * fetch_record_bytes(s, &slot);
    if (nkeys > 0 && !dev_keys) return set_err(DML_E_INVALID_ARG, "null keys");
    if (((uintptr_t)dev_keys & 7) != 0) return set_err(DML_E_INVALID_ARG, "fetch keys are not 8-byte aligned");
    return fetch_device_impl(s, dev_keys, nkeys, 0, dev_out, cap, out_len, (hipStream_t)stream);
}

int dml_store_fetch_range_device(dml_store* s, int64_t first_key, int64_t last_key, void* dev_out, int64_t cap,
                                 int64_t* out_len, void* stream) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    if (!out_len) return set_err(DML_E_INVALID_ARG, "null out_len");
    // KeyRange.intersect (KeyRange.java:124-136): clip to the shard, ascending
    const int64_t lo = std::max(first_key, s->first), hi = std::min(last_key, s->last);
    const int64_t nkeys = lo <= hi ? hi - lo + 1 : 0;
    int slot;
    *out_len = nkeys * fetch_record_bytes(s, &slot);
    return fetch_device_impl(s, nullptr, nkeys, lo, dev_out, cap, out_len, (hipStream_t)stream);
}

// Rows [lo, hi] (local indices), big-endian, row-major: DataOutputStream.write{Float,Int,Double}.
static int write_rows_be(dml_store* s, int64_t lo, int64_t hi, uint8_t* out) {
    if (hi < lo) return DML_OK;
    const int64_t n = (hi - lo + 1) * s->cols;
    const size_t bytes = (size_t)n * (size_t)s->V;
    if (int rc = ensure_scratch(s, bytes)) return rc;
    HIPCHK(launch_bswap(s->V, (const uint8_t*)s->data + (size_t)lo * s->cols * s->V, s->dscr, n, s->stream));
    return d2h(s, out, s->dscr, bytes);
}

// The first `nelem` elements from row lo on, from big-endian bytes (DataInputStream.read*).
static int read_elems_be(dml_store* s, int64_t lo, int64_t nelem, const uint8_t* in) {
    if (nelem <= 0) return DML_OK;
    const size_t bytes = (size_t)nelem * (size_t)s->V;
    if (int rc = ensure_scratch(s, bytes)) return rc;
    if (int rc = h2d(s, s->dscr, in, bytes)) return rc;
    HIPCHK(launch_bswap(s->V, s->dscr, (uint8_t*)s->data + (size_t)lo * s->cols * s->V, nelem, s->stream));
    return drain(s);
}

int dml_store_write_all(dml_store* s, uint8_t* out_be, int64_t cap, int64_t* out_len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    const int64_t bytes = s->rows * s->cols * s->V;
    if (out_len) *out_len = bytes;
    if (!out_be || cap < bytes) return set_err(DML_E_CAPACITY, "writeAll buffer too small");
    return write_rows_be(s, 0, s->rows - 1, out_be);
}

int dml_store_read_all(dml_store* s, const uint8_t* in_be, int64_t len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    const int64_t n = s->rows * s->cols;
    if (len < 0 || (len > 0 && !in_be)) return set_err(DML_E_INVALID_ARG, "bad readAll arguments");
    // readFloat past the end throws EOFException after the elements before it were assigned
    const int64_t avail = std::min(n, len / s->V);
    if (int rc = read_elems_be(s, 0, avail, in_be)) return rc;
    if (avail < n) return set_err(DML_E_TRUNCATED, "readAll: stream shorter than the shard");
    return DML_OK;
}

int dml_store_sync_to(dml_store* s, int32_t from_row, int32_t to_row, uint8_t* out_be, int64_t cap,
                      int64_t* out_len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    if (!out_len) return set_err(DML_E_INVALID_ARG, "null out_len");
    *out_len = 0;
    if (to_row < from_row) return DML_OK;  // the loop body never runs
    // localData[i] for i = from..to: a negative row throws before any write, a row
    // past the shard after the rows before it were written (ArrayIndexOutOfBounds)
    if (from_row < 0) return set_err(DML_E_KEY_OUT_OF_SHARD, "syncTo: negative row");
    const int64_t hi = std::min<int64_t>(to_row, s->rows - 1);
    const int64_t bytes = hi >= from_row ? (hi - from_row + 1) * s->cols * s->V : 0;
    if (!out_be || cap < bytes) {
        *out_len = bytes;
        return set_err(DML_E_CAPACITY, "syncTo buffer too small");
    }
    if (int rc = write_rows_be(s, from_row, hi, out_be)) return rc;
    *out_len = bytes;
    if (to_row >= s->rows) return set_err(DML_E_KEY_OUT_OF_SHARD, "syncTo: row past the shard");
    return DML_OK;
}

int dml_store_sync_from(dml_store* s, int32_t from_row, int32_t to_row, const uint8_t* in_be, int64_t len) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    if (len < 0 || (len > 0 && !in_be)) return set_err(DML_E_INVALID_ARG, "bad syncFrom arguments");
    if (to_row < from_row) return DML_OK;
    if (from_row < 0) return set_err(DML_E_KEY_OUT_OF_SHARD, "syncFrom: negative row");
    // elements assigned in order until the stream ends (EOF) or a row falls past the shard
    const int64_t hi = std::min<int64_t>(to_row, s->rows - 1);
    const int64_t want = hi >= from_row ? (hi - from_row + 1) * s->cols : 0;
    const int64_t avail = std::min(want, len / s->V);
    if (int rc = read_elems_be(s, from_row, avail, in_be)) return rc;
    if (avail < want) return set_err(DML_E_TRUNCATED, "syncFrom: stream shorter than the rows");
    if (to_row >= s->rows) return set_err(DML_E_KEY_OUT_OF_SHARD, "syncFrom: row past the shard");
    return DML_OK;
}

int dml_host_alloc(int64_t bytes, void** host_ptr) {
    if (bytes < 0 || !host_ptr) return set_err(DML_E_INVALID_ARG, "bad host alloc arguments");
    *host_ptr = nullptr;
    HIPCHK(hipHostMalloc(host_ptr, (size_t)std::max<int64_t>(bytes, 1), hipHostMallocDefault));
    return DML_OK;
}

void dml_host_free(void* host_ptr) {
    if (host_ptr) (void)hipHostFree(host_ptr);
}

}  // extern "C"

// The owner's side of dml_group_pull (dml_group.hip): the records of `nkeys` device keys, all
// inside the shard (the requesters' partition put them there), encoded by k_fetch_vec into
// dev_out on the apply stream; nothing is waited for. Entry as every read's (begin_call), but
// what it reports does not stop the encode: the peers have sized their receives, so a shard
// with a deferred error, or in its sticky error state, answers with its bytes as they stand,
// and the error is returned behind the launch.
namespace dml {
int store_pull_encode(dml_store* s, const int64_t* dev_keys, int64_t nkeys, void* dev_out) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    const int held = begin_call(s);
    if (nkeys <= 0) return held;
    int value_slot;
    const int64_t rec = fetch_record_bytes(s, &value_slot);
    if (int rc = ensure_fetch_record(s)) return rc;
    const int variant = (s->fetch_kernel & 0xFF) == 2 ? (int)(s->fetch_kernel >> 8) : 0;
    HIPCHK(launch_fetch_vec(vtype_of(s->desc), s->data, s->adagrad ? s->alpha : nullptr, s->cols, dev_keys, 0, nkeys,
                            s->first, s->last, (uint8_t*)dev_out, rec, s->K, value_slot, s->fbad_dev, variant, s->stream));
    return held;
}

int store_fetch_record_bytes(dml_store* s, int64_t* rec) {
    if (int rc = check_store(s)) return rc;
    int value_slot;
    *rec = fetch_record_bytes(s, &value_slot);
    return DML_OK;
}
}  // namespace dml

// dml_store_owner.hip — what a shard group drives on an owner's store: the applies and
// commits of slices that arrive in HBM (dml_store_apply_dense_device, dml_store_assign_*_device,
// dml_store_apply_adagrad_moments_device), the plane push of a worker on the store's own GPU
// (dml_store_push_planes_device, dml_store_push_elems_device), the compact-row push and split
// (dml_store_push_compact_rows_device, dml_compact_rows_split) and the dml::store_* calls of dml_group.hip. Pushes
// before them are retired first; an earlier call's verdict is read only once it has landed.
#include "dml_store_impl.h"

using namespace dml;
using namespace dml::detail;

// The owner's commit of a chained AdaGrad slice, rows [row0, row0 + nrows) of the shard
// (dml_store_assign_adagrad_device is the whole shard; the group commits a slice sub-chunk
// by sub-chunk, as it travelled). rec == null leaves the running maxDelta alone.
namespace dml {
int store_assign_adagrad(dml_store* s, int64_t row0, int64_t nrows, const void* data, const void* delta,
                         const void* marks, const void* rec) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    if (row0 < 0 || nrows < 0 || row0 > s->rows || nrows > s->rows - row0)
        return set_err(DML_E_INVALID_ARG, "assign: bad row range");
    // every accepted push is retired first, as in dml_store_assign_dense_device
    if (int rc = retire_all(s)) return rc;
    if (int rc = failed(s)) return rc;
    if (nrows == 0 && !rec) return DML_OK;
    const int64_t e0 = row0 * s->cols;
    HIPCHK(launch_chain_ada_commit((float*)s->data + e0, s->delta + e0, s->alpha + e0, rec ? s->md : nullptr,
                                   (const float*)data, (const float*)delta, (const uint32_t*)marks,
                                   (const MaxDelta*)rec, nrows, s->cols, ada_args(s), s->stream));
    return DML_OK;
}

int store_chain_i32_record(dml_store* s, void** dev_rec) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->is_matrix || s->adagrad || !s->desc.dense_column || vtype_of(s->desc) != kI32)
        return set_err(DML_E_UNSUPPORTED, "not a dense int32 matrix store");
    if (int rc = s->crec.ensure(s->stream)) return rc;
    *dev_rec = s->crec.dev;  // step 0 of a chained call seeds its slice's record from the sticky one
    return DML_OK;
}

int store_chain_i32_collect(dml_store* s, bool block) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = collect_chain_check(s, block)) return rc;
    return failed(s);
}

int store_adagrad_ptrs(dml_store* s, float** delta, void** maxdelta) {
    if (int rc = check_store(s)) return rc;
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    *delta = s->delta;
    *maxdelta = s->md;
    return DML_OK;
}
}  // namespace dml

extern "C" {

int dml_store_apply_dense_device(dml_store* s, const void* dev_src, int64_t elems) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    // pushes before it are retired (an error there stops the store like the
    // reference); the previous owner apply's check is read only if it has finished:
    // blocking on it would serialize the sharded int32 pipeline
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (!dev_src || elems != s->rows * s->cols) return set_err(DML_E_INVALID_ARG, "apply size mismatch");
    std::pair<hipEvent_t, hipEvent_t> ev{};
    if (s->timing) {
        ev = ev_pair(s);
        HIPCHK(hipEventRecord(ev.first, s->stream));
    }
    if (vtype_of(s->desc) == kI32) {
        // IntMatrixStore: check the final counters (IntMatrixStore.java:174-176); the
        // kernel skips itself once an earlier apply left a negative (sticky neg.dev, closed
        // until dml_store_clear_error)
        if (int rc = s->neg.ensure(s->stream)) return rc;
        HIPCHK(launch_apply_dense_i32chk((int32_t*)s->data, (const int32_t*)dev_src, elems, s->neg.dev, s->stream));
        if (int rc = s->neg.post(s->stream)) return rc;
    } else {
        HIPCHK(launch_apply_dense(vtype_of(s->desc), s->data, dev_src, elems, s->stream));
    }
    if (s->timing) {
        HIPCHK(hipEventRecord(ev.second, s->stream));
        s->ev_used.push_back(ev);
    }
    return DML_OK;
}

// The plane push (dml_push_planes.hip): refusals first, with nothing changed;
// then the owner applies' entry; then the coalescer's order stage on the caller's stream and the
// sums into the shard on the apply stream (dml::co_push_planes).
int dml_store_push_planes_device(dml_store* s, dml_coalescer* c, const int64_t* dev_keys, int64_t n,
                                 const void* dev_values, void* stream) {
    if (int rc = check_store(s)) return rc;
    if (!c) return set_err(DML_E_INVALID_ARG, "null coalescer");
    Entry in(s);
    if (n < 0) return set_err(DML_E_INVALID_ARG, "negative occurrence count");
    if (n > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "lists of 2^31 occurrences and more");
    if (n > 0 && (!dev_keys || !dev_values)) return set_err(DML_E_INVALID_ARG, "null keys or values plane");
    if (((uintptr_t)dev_keys & 7) != 0) return set_err(DML_E_INVALID_ARG, "push keys are not 8-byte aligned");
    if (((uintptr_t)dev_values & 3) != 0) return set_err(DML_E_INVALID_ARG, "push plane is not 4-byte aligned");
    if (co_device(c) != s->device) return set_err(DML_E_INVALID_ARG, "the coalescer belongs to another device");
    if (s->is_matrix && !s->desc.dense_column)
        return set_err(DML_E_UNSUPPORTED, "sparse-column matrix rows are not supported (SURVEY defect 3)");
    if (vtype_of(s->desc) == kI32)
        return set_err(DML_E_UNSUPPORTED, "plane pushes into int32 stores: their checked adds need a rollback");
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (n == 0) return DML_OK;
    if (!s->fbad_dev) {  // the running call's lowest refused index, then the sticky verdict: a device fetch's
        HIPCHK(hipMalloc((void**)&s->fbad_dev, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->fbad_dev, 0xFF, sizeof(unsigned long long), s->stream));
    }
    if (int rc = s->fver.ensure(s->stream)) return rc;
    if (s->adagrad && s->cand_n < kPushCands) {  // one candidate per block of the call's kernels
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipFree(s->cand));
        s->cand = nullptr;
        s->cand_n = 0;
        HIPCHK(hipMalloc((void**)&s->cand, sizeof(DeltaCand) * (size_t)(kPushCands + kMdParts)));
        s->cand_n = kPushCands;
    }
    const int64_t cols = s->is_matrix ? s->cols : 1;
    PushSink sk{};
    sk.data = (uint8_t*)s->data;
    sk.delta = s->delta;
    sk.alpha = s->alpha;
    sk.cand = s->cand;
    sk.md = s->adagrad ? s->md : nullptr;
    sk.initial_alpha = s->initial_alpha;
    sk.min_alpha = s->min_alpha;
    sk.factor = s->factor;
    sk.first = s->first;
    sk.last = s->last;
    sk.cols = (int32_t)cols;
    sk.bad = s->fbad_dev;
    sk.verdict = s->fver.dev;
    sk.apply = s->stream;
    if (int rc = co_push_planes(c, vtype_of(s->desc), cols * s->V, dev_keys, n, dev_values, sk, stream)) return rc;
    if (int rc = s->fver.post(s->stream)) return rc;
    if (stream) return DML_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    return collect_fetch_check(s, true);
}

// The element push (dml_push_elems.hip): the plane push's refusals, entry and
// streams, with the int32 stores' checked adds as the sink (dml::co_push_elems).
int dml_store_push_elems_device(dml_store* s, dml_coalescer* c, const int64_t* dev_keys, int64_t n, int32_t per_occ,
                                const int32_t* dev_cols, const int32_t* dev_vals, void* stream) {
    if (int rc = check_store(s)) return rc;
    if (!c) return set_err(DML_E_INVALID_ARG, "null coalescer");
    Entry in(s);
    if (n < 0) return set_err(DML_E_INVALID_ARG, "negative occurrence count");
    if (n > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "lists of 2^31 occurrences and more");
    if (per_occ < 1 || per_occ > DML_COALESCE_ELEMS_MAX_PER_OCC)
        return set_err(DML_E_INVALID_ARG, "per_occ outside 1 .. DML_COALESCE_ELEMS_MAX_PER_OCC");
    if (((uintptr_t)dev_keys & 7) != 0) return set_err(DML_E_INVALID_ARG, "push keys are not 8-byte aligned");
    if ((((uintptr_t)dev_cols | (uintptr_t)dev_vals) & 3) != 0)
        return set_err(DML_E_INVALID_ARG, "columns or values are not 4-byte aligned");
    if (co_device(c) != s->device) return set_err(DML_E_INVALID_ARG, "the coalescer belongs to another device");
    if (vtype_of(s->desc) != kI32 || s->adagrad)
        return set_err(DML_E_UNSUPPORTED, "element updates are int32 only: float sums depend on their order");
    if (s->is_matrix && !s->desc.dense_column)
        return set_err(DML_E_UNSUPPORTED, "sparse-column matrix rows are not supported (SURVEY defect 3)");
    if (!s->is_matrix && dev_cols) return set_err(DML_E_INVALID_ARG, "an array store's elements have no column");
    if (n > 0 && (!dev_keys || !dev_vals || (s->is_matrix && !dev_cols)))
        return set_err(DML_E_INVALID_ARG, "null keys, columns or values");
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (n == 0) return DML_OK;
    if (!s->fbad_dev) {  // as a device fetch's
        HIPCHK(hipMalloc((void**)&s->fbad_dev, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->fbad_dev, 0xFF, sizeof(unsigned long long), s->stream));
    }
    if (!s->pe_cell) {
        HIPCHK(hipMalloc((void**)&s->pe_cell, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->pe_cell, 0xFF, sizeof(unsigned long long), s->stream));
    }
    if (int rc = s->fver.ensure(s->stream)) return rc;
    if (int rc = s->neg.ensure(s->stream)) return rc;
    ElemSink sk{};
    sk.data = (int32_t*)s->data;
    sk.first = s->first;
    sk.last = s->last;
    sk.cols = s->is_matrix ? s->cols : 1;
    sk.cell = s->pe_cell;
    sk.bad = s->fbad_dev;
    sk.neg = s->neg.dev;
    sk.fver = s->fver.dev;
    sk.apply = s->stream;
    if (int rc = co_push_elems(c, dev_keys, n, per_occ, dev_cols, dev_vals, sk, stream)) return rc;
    if (int rc = s->fver.post(s->stream)) return rc;
    if (int rc = s->neg.post(s->stream)) return rc;
    if (stream) return DML_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    return collect_apply_check(s, true);
}

// The compact-row push (dml_compact_rows.hip): the element push's entry, streams
// and sink, with no coalescer and no host wait: the list arrives ordered and summed, and what is
// not known about it (its form) is checked on the device.
int dml_store_push_compact_rows_device(dml_store* s, const int64_t* dev_keys, const int32_t* dev_ptr,
                                       const int32_t* dev_ecol, const int32_t* dev_eval, int64_t m, void* stream) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (m < 0) return set_err(DML_E_INVALID_ARG, "negative row count");
    if (m > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "lists of 2^31 rows and more");
    if (((uintptr_t)dev_keys & 7) != 0) return set_err(DML_E_INVALID_ARG, "push keys are not 8-byte aligned");
    if ((((uintptr_t)dev_ptr | (uintptr_t)dev_ecol | (uintptr_t)dev_eval) & 3) != 0)
        return set_err(DML_E_INVALID_ARG, "ptr, columns or values are not 4-byte aligned");
    if (vtype_of(s->desc) != kI32 || s->adagrad || !s->is_matrix)
        return set_err(DML_E_UNSUPPORTED, "compact rows are IntMatrixStore updates: the record route serves the rest");
    if (!s->desc.dense_column)
        return set_err(DML_E_UNSUPPORTED, "sparse-column matrix rows are not supported (SURVEY defect 3)");
    if (m > 0 && (!dev_keys || !dev_ptr || !dev_ecol || !dev_eval))
        return set_err(DML_E_INVALID_ARG, "null keys, ptr, columns or values");
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (m == 0) return DML_OK;
    if (!s->fbad_dev) {  // as a device fetch's
        HIPCHK(hipMalloc((void**)&s->fbad_dev, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->fbad_dev, 0xFF, sizeof(unsigned long long), s->stream));
    }
    if (!s->pe_cell) {
        HIPCHK(hipMalloc((void**)&s->pe_cell, sizeof(unsigned long long)));
        HIPCHK(hipMemsetAsync(s->pe_cell, 0xFF, sizeof(unsigned long long), s->stream));
    }
    if (m > s->cr_cap) {  // only a list longer than every one before it: the kernels of earlier calls end first
        if (s->cr_scratch) {
            HIPCHK(hipStreamSynchronize(s->stream));
            HIPCHK(hipFree(s->cr_scratch));
        }
        s->cr_scratch = nullptr;
        s->cr_cap = 0;
        const int64_t cap = m + m / 4;
        HIPCHK(hipMalloc((void**)&s->cr_scratch, 16 + (size_t)cap * 4));
        HIPCHK(hipMemsetAsync(s->cr_scratch, 0xFF, 8, s->stream));    // the format cell: open
        HIPCHK(hipMemsetAsync(s->cr_scratch + 8, 0, 8, s->stream));   // the route word
        s->cr_cap = cap;
    }
    if (int rc = s->fver.ensure(s->stream)) return rc;
    if (int rc = s->neg.ensure(s->stream)) return rc;
    PushCompactP a{};
    a.keys = dev_keys;
    a.ptr = dev_ptr;
    a.ecol = dev_ecol;
    a.eval = dev_eval;
    a.m = m;
    a.nslice = ((int64_t)s->cols + DML_COALESCE_ELEMS_SLICE - 1) / DML_COALESCE_ELEMS_SLICE;
    a.ncols = s->cols;
    a.form = (unsigned long long*)s->cr_scratch;
    a.route = (uint32_t*)(s->cr_scratch + 8);
    a.list = (uint32_t*)(s->cr_scratch + 16);
    a.sink.data = (int32_t*)s->data;
    a.sink.first = s->first;
    a.sink.last = s->last;
    a.sink.cols = s->cols;
    a.sink.cell = s->pe_cell;
    a.sink.bad = s->fbad_dev;
    a.sink.neg = s->neg.dev;
    a.sink.fver = s->fver.dev;
    a.sink.apply = s->stream;
    if (stream && (hipStream_t)stream != s->stream) {  // the list is complete on `stream`: no host wait
        if (!s->cr_handoff) HIPCHK(hipEventCreateWithFlags(&s->cr_handoff, hipEventDisableTiming));
        HIPCHK(hipEventRecord(s->cr_handoff, (hipStream_t)stream));
        HIPCHK(hipStreamWaitEvent(s->stream, s->cr_handoff, 0));
    }
    HIPCHK(launch_push_compact(a, s->stream));
    if (int rc = s->fver.post(s->stream)) return rc;
    if (int rc = s->neg.post(s->stream)) return rc;
    if (stream) return DML_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    return collect_apply_check(s, true);
}

// The batch form (dml_compact_rows_batch.hip): the single call's entry, streams and
// sticky verdicts. The non-empty runs go into the kernel arguments in list order (an empty run is a
// single call that launches nothing), so nothing is uploaded and the host never waits.
int dml_store_push_compact_rows_batch_device(dml_store* s, int32_t runs, const int64_t* const* dev_keys,
                                             const int32_t* const* dev_ptr, const int32_t* const* dev_ecol,
                                             const int32_t* const* dev_eval, const int64_t* m, void* stream) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (runs < 0 || runs > DML_COMPACT_ROWS_BATCH_MAX_RUNS)
        return set_err(DML_E_INVALID_ARG, "runs outside 0 .. DML_COMPACT_ROWS_BATCH_MAX_RUNS");
    if (runs > 0 && (!dev_keys || !dev_ptr || !dev_ecol || !dev_eval || !m))
        return set_err(DML_E_INVALID_ARG, "null run table");
    PushCompactBatchP a{};
    int64_t total = 0;
    for (int32_t q = 0; q < runs; ++q) {
        if (m[q] < 0 || m[q] > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "a run's row count outside 0 .. 2^31 - 1");
        if (m[q] == 0) continue;
        if (!dev_keys[q] || !dev_ptr[q] || !dev_ecol[q] || !dev_eval[q])
            return set_err(DML_E_INVALID_ARG, "null keys, ptr, columns or values in a run with rows");
        if (((uintptr_t)dev_keys[q] & 7) != 0) return set_err(DML_E_INVALID_ARG, "push keys are not 8-byte aligned");
        if ((((uintptr_t)dev_ptr[q] | (uintptr_t)dev_ecol[q] | (uintptr_t)dev_eval[q]) & 3) != 0)
            return set_err(DML_E_INVALID_ARG, "ptr, columns or values are not 4-byte aligned");
        total += m[q];
        if (total > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "batches of 2^31 rows and more");
        a.run[a.runs] = CompactRun{dev_keys[q], dev_ptr[q], dev_ecol[q], dev_eval[q]};
        a.off[++a.runs] = (uint32_t)total;
    }
    if (vtype_of(s->desc) != kI32 || s->adagrad || !s->is_matrix)
        return set_err(DML_E_UNSUPPORTED, "compact rows are IntMatrixStore updates: the record route serves the rest");
    if (!s->desc.dense_column)
        return set_err(DML_E_UNSUPPORTED, "sparse-column matrix rows are not supported (SURVEY defect 3)");
    // a negative counter's order word: (run x rows + row) x cols + col, below kNoPos
    if ((unsigned __int128)std::max(a.runs, 1) * (unsigned __int128)s->rows * (unsigned __int128)s->cols >= (unsigned __int128)kNoPos)
        return set_err(DML_E_UNSUPPORTED, "runs x rows x cols does not fit 64 bits: make several calls");
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (a.runs == 0) return DML_OK;
    if (!s->crb_cells) {
        HIPCHK(hipMalloc((void**)&s->crb_cells, sizeof(unsigned long long) * kCrbCells));
        HIPCHK(hipMemsetAsync(s->crb_cells, 0xFF, sizeof(unsigned long long) * kCrbCells, s->stream));  // all open
    }
    if (int rc = s->fver.ensure(s->stream)) return rc;
    if (int rc = s->neg.ensure(s->stream)) return rc;
    a.ncols = s->cols;
    a.nslice = ((int64_t)s->cols + DML_COALESCE_ELEMS_SLICE - 1) / DML_COALESCE_ELEMS_SLICE;
    a.cells = s->crb_cells;
    a.sink.data = (int32_t*)s->data;
    a.sink.first = s->first;
    a.sink.last = s->last;
    a.sink.cols = s->cols;
    a.sink.neg = s->neg.dev;
    a.sink.fver = s->fver.dev;
    a.sink.apply = s->stream;
    if (stream && (hipStream_t)stream != s->stream) {  // the runs are complete on `stream`: no host wait
        if (!s->cr_handoff) HIPCHK(hipEventCreateWithFlags(&s->cr_handoff, hipEventDisableTiming));
        HIPCHK(hipEventRecord(s->cr_handoff, (hipStream_t)stream));
        HIPCHK(hipStreamWaitEvent(s->stream, s->cr_handoff, 0));
    }
    HIPCHK(launch_push_compact_batch(a, s->stream));
    if (int rc = s->fver.post(s->stream)) return rc;
    if (int rc = s->neg.post(s->stream)) return rc;
    if (stream) return DML_OK;
    HIPCHK(hipStreamSynchronize(s->stream));
    return collect_apply_check(s, true);
}

int dml_compact_rows_split(const int64_t* dev_keys, int64_t m, const int32_t* dev_ptr, int64_t total_rows,
                           int32_t world, int64_t* dev_row_off, int64_t* dev_entry_off, int32_t* dev_ptr_out,
                           void* stream) {
    if (m < 0 || m > 0x7FFFFFFFll) return set_err(DML_E_INVALID_ARG, "row count outside 0 .. 2^31 - 1");
    if (total_rows < 1 || world < 1 || world > DML_COMPACT_ROWS_MAX_WORLD)
        return set_err(DML_E_INVALID_ARG, "total_rows < 1, or world outside 1 .. DML_COMPACT_ROWS_MAX_WORLD");
    if (!dev_ptr || !dev_row_off || !dev_entry_off || !dev_ptr_out || (m > 0 && !dev_keys))
        return set_err(DML_E_INVALID_ARG, "null keys, ptr or output pointer");
    if ((((uintptr_t)dev_keys | (uintptr_t)dev_row_off | (uintptr_t)dev_entry_off) & 7) != 0)
        return set_err(DML_E_INVALID_ARG, "keys or offsets are not 8-byte aligned");
    if ((((uintptr_t)dev_ptr | (uintptr_t)dev_ptr_out) & 3) != 0)
        return set_err(DML_E_INVALID_ARG, "ptr arrays are not 4-byte aligned");
    hipPointerAttribute_t at{};  // the kernels run where the list lies
    HIPCHK(hipPointerGetAttributes(&at, dev_ptr));
    DeviceGuard g(at.device);
    HIPCHK(launch_compact_split(dev_keys, m, dev_ptr, total_rows, world, dev_row_off, dev_entry_off, dev_ptr_out,
                                (hipStream_t)stream));
    if (!stream) HIPCHK(hipStreamSynchronize(nullptr));
    return DML_OK;
}

int dml_store_assign_dense_device(dml_store* s, const void* dev_src, int64_t elems) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->is_matrix || s->adagrad || !s->desc.dense_column)
        return set_err(DML_E_UNSUPPORTED, "assign: plain dense-column matrices (f32 / f64 / i32)");
    // every accepted push is retired first: s->data is then the buffer the last of
    // them wrote (a speculative chunk commits the store's second buffer at its retire)
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (!dev_src || elems != s->rows * s->cols) return set_err(DML_E_INVALID_ARG, "assign size mismatch");
    HIPCHK(hipMemcpyAsync(s->data, dev_src, (size_t)elems * (size_t)s->V, hipMemcpyDeviceToDevice, s->stream));
    return DML_OK;
}

int dml_store_assign_dense_i32_device(dml_store* s, const void* dev_src, int64_t elems, const void* dev_record) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->is_matrix || s->adagrad || !s->desc.dense_column || vtype_of(s->desc) != kI32)
        return set_err(DML_E_UNSUPPORTED,
                       "assign with a verdict record: dense int32 matrices (fp32 / fp64: dml_store_assign_dense_device)");
    if (int rc = retire_all(s)) return rc;
    if (int rc = collect_apply_check(s, false)) return rc;
    if (int rc = failed(s)) return rc;
    if (!dev_src || !dev_record || elems != s->rows * s->cols) return set_err(DML_E_INVALID_ARG, "assign size mismatch");
    if ((uintptr_t)dev_record & 7u) return set_err(DML_E_INVALID_ARG, "verdict record is not 8-byte aligned");
    if (int rc = s->crec.ensure(s->stream)) return rc;
    // the slice as it came home: a closed one holds the adds up to the failing one
    HIPCHK(hipMemcpyAsync(s->data, dev_src, (size_t)elems * (size_t)s->V, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(launch_chain_i32_merge(s->crec.dev, (const ChainI32Rec*)dev_record, s->stream));
    return s->crec.post(s->stream);
}

int dml_store_assign_adagrad_device(dml_store* s, const void* dev_data, const void* dev_delta, const void* dev_marks,
                                    const void* dev_maxdelta_record) {
    if (int rc = check_store(s)) return rc;
    if (!dev_data || !dev_delta || !dev_marks || !dev_maxdelta_record)
        return set_err(DML_E_INVALID_ARG, "assign: null plane or record");
    return store_assign_adagrad(s, 0, s->rows, dev_data, dev_delta, dev_marks, dev_maxdelta_record);
}

int dml_store_apply_adagrad_moments_device(dml_store* s, const void* dev_src, int64_t rows) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (!s->adagrad) return set_err(DML_E_UNSUPPORTED, "not an AdaGrad store");
    if (!dev_src || rows != s->rows) return set_err(DML_E_INVALID_ARG, "moments size mismatch");
    if (s->cols % 4) return set_err(DML_E_UNSUPPORTED, "two-moment apply: rows of whole 16-B vectors");
    if (int rc = retire_all(s)) return rc;
    if (int rc = failed(s)) return rc;
    if (s->cand_n < kMomentBlocks) {  // one candidate per apply block
        HIPCHK(hipStreamSynchronize(s->stream));
        HIPCHK(hipFree(s->cand));
        s->cand = nullptr;
        HIPCHK(hipMalloc((void**)&s->cand, sizeof(DeltaCand) * (size_t)(kMomentBlocks + kMdParts)));
        s->cand_n = kMomentBlocks;
    }
    std::pair<hipEvent_t, hipEvent_t> ev{};
    if (s->timing) ev = ev_pair(s);
    HIPCHK(launch_ada_moments((float*)s->data, (const float*)dev_src, s->rows, s->cols, ada_args(s), s->md, s->first,
                              s->stream, LaunchEv{ev.first, ev.second}));
    if (s->timing) s->ev_used.push_back(ev);
    s->kname = g_kernel_name;
    return DML_OK;
}

}  // extern "C"

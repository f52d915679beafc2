// dml_store_owner.hip — what a shard group drives on an owner's store: the applies and
// commits of slices that arrive in HBM (dml_store_apply_dense_device, dml_store_assign_*_device,
// dml_store_apply_adagrad_moments_device) and the dml::store_* calls of dml_group.hip. Pushes
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

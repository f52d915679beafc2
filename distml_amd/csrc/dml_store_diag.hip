// dml_store_diag.hip — what initialises, measures and tunes a store beside its data path:
// DataStore.rand() (with the java.util.Random model DoubleMatrixStore needs), the synthetic
// data calls (dml_synth_*), the knobs, the kernel name and timing, and the dml_diag_* floors.
#include "dml_store_impl.h"
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace dml;
using namespace dml::detail;

namespace {

// java.util.Random as its specification defines it: 48-bit LCG (multiplier
// 0x5DEECE66D, addend 0xB), setSeed's scramble, nextDouble from 26 + 27 bits, and
// nextGaussian by the polar method with StrictMath.log (fdlibm's e_log.c, below)
// and StrictMath.sqrt (IEEE). Used by dml_store_rand for DoubleMatrixStore.rand().
struct JavaRandom {
    uint64_t x;
    bool have = false;
    double spare = 0.0;
    explicit JavaRandom(int64_t seed) : x(((uint64_t)seed ^ 0x5DEECE66DULL) & kMask) {}
    static constexpr uint64_t kMask = (1ULL << 48) - 1;
    int32_t next(int bits) {
        x = (x * 0x5DEECE66DULL + 0xBULL) & kMask;
        return (int32_t)(uint32_t)(x >> (48 - bits));
    }
    double next_double() {
        const int64_t hi = next(26);
        return (double)((hi << 27) + next(27)) * 0x1.0p-53;
    }
    static double strict_log(double v);
    double next_gaussian() {
        if (have) {
            have = false;
            return spare;
        }
        double a, b, q;
        do {
            a = 2 * next_double() - 1;
            b = 2 * next_double() - 1;
            q = a * a + b * b;
        } while (q >= 1 || q == 0);
        const double m = std::sqrt(-2 * strict_log(q) / q);
        spare = b * m;
        have = true;
        return a * m;
    }
};

// fdlibm __ieee754_log: reduce to x = 2^k (1 + f) with sqrt(2)/2 < 1 + f < sqrt(2),
// then log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)), s = f / (2 + f), R a degree-14
// minimax polynomial in s (its published coefficients Lg1..Lg7).
double JavaRandom::strict_log(double v) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                     two54 = 1.80143985094819840000e+16;
    constexpr double L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01, L3 = 2.857142874366239149e-01,
                     L4 = 2.222219843214978396e-01, L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
                     L7 = 1.479819860511658591e-01;
    uint64_t u;
    memcpy(&u, &v, 8);
    int32_t hx = (int32_t)(u >> 32), k = 0;
    if (hx < 0x00100000) {
        if (((hx & 0x7fffffff) | (int32_t)(uint32_t)u) == 0) return -std::numeric_limits<double>::infinity();
        if (hx < 0) return std::numeric_limits<double>::quiet_NaN();
        k = -54;
        v *= two54;
        memcpy(&u, &v, 8);
        hx = (int32_t)(u >> 32);
    }
    if (hx >= 0x7ff00000) return v + v;
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int32_t i0 = (hx + 0x95f64) & 0x100000;
    u = ((uint64_t)(uint32_t)(hx | (i0 ^ 0x3ff00000)) << 32) | (u & 0xffffffffULL);
    memcpy(&v, &u, 8);
    k += i0 >> 20;
    const double f = v - 1.0, dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (L2 + w * (L4 + w * L6));
    const double t2 = z * (L1 + w * (L3 + w * (L5 + w * L7)));
    const double R = t2 + t1;
    if (((hx - 0x6147a) | (0x6b851 - hx)) > 0) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// One row of DoubleMatrixStore.rand() (DoubleMatrixStore.java:196-206).
void java_unit_abs_gaussian_row(JavaRandom& jr, double* row, int64_t cols) {
    double sum = 0.0;
    for (int64_t j = 0; j < cols; ++j) {
        row[j] = std::fabs(jr.next_gaussian());
        sum += row[j] * row[j];
    }
    sum = std::sqrt(sum);
    for (int64_t j = 0; j < cols; ++j) row[j] = row[j] / sum;
}

// One launch of a dml_diag_* floor with a fresh event pair in its packet: *ms = its time.
template <typename Launch>
int timed_launch(float* ms, Launch launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0));
    hipError_t e = hipEventCreate(&e1);
    if (e == hipSuccess) e = launch(LaunchEv{e0, e1});
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (e != hipSuccess) return set_err(DML_E_HIP, hipGetErrorString(e));
    if (ms) *ms = t;
    return DML_OK;
}
}  // namespace

extern "C" {

int dml_store_stream(dml_store* s, void** stream) {
    if (int rc = check_store(s)) return rc;
    if (!stream) return set_err(DML_E_INVALID_ARG, "null out");
    *stream = (void*)s->stream;
    return DML_OK;
}

int dml_store_set_timing(dml_store* s, int32_t enable) {
    if (int rc = check_store(s)) return rc;
    std::lock_guard<std::mutex> lk(s->mu);
    s->timing = enable != 0;
    s->timing_every = enable > 1 ? enable : 1;
    s->timing_k = 0;
    return DML_OK;
}

// DML_KNOB_INDEX_CUS: the index stream (the next chunk's key index / sparse partition)
// on k of the device's CUs and the apply stream on the others (k = 0: both streams on
// every CU, the default). pattern 0 spreads the k CUs evenly over the CU numbering,
// 1 takes the first k. Caller holds s->mu.
static int set_cu_split(dml_store* s, int k, int pattern) {
    DeviceGuard g(s->device);
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s->device));
    if (k < 0 || k >= ncu || pattern < 0 || pattern > 1) return set_err(DML_E_INVALID_ARG, "bad CU split");
    if (int rc = begin_call(s)) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipStreamSynchronize(s->istream));
    const int words = (ncu + 31) / 32;
    std::vector<uint32_t> mi((size_t)words, 0u), ma((size_t)words, 0u);
    for (int c = 0; c < ncu; ++c) {
        const bool idx = k > 0 && (pattern == 1 ? c < k : (int64_t)c * k % ncu < k);
        (idx ? mi : ma)[(size_t)(c / 32)] |= 1u << (c % 32);
    }
    hipStream_t ns = nullptr, ni = nullptr;
    if (k == 0) {
        HIPCHK(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&ni, hipStreamNonBlocking));
    } else {
        HIPCHK(hipExtStreamCreateWithCUMask(&ns, (uint32_t)words, ma.data()));
        HIPCHK(hipExtStreamCreateWithCUMask(&ni, (uint32_t)words, mi.data()));
    }
    (void)hipStreamDestroy(s->stream);
    (void)hipStreamDestroy(s->istream);
    s->stream = ns;
    s->istream = ni;
    return DML_OK;
}

int dml_diag_store_knob(dml_store* s, int32_t knob, int64_t value) {
    if (int rc = check_store(s)) return rc;
    if (value < 0) return set_err(DML_E_INVALID_ARG, "negative knob value");
    std::lock_guard<std::mutex> lk(s->mu);
    switch (knob) {
        case DML_KNOB_IDENT_FULL_MIN_BYTES: s->ident_full_min = value; return DML_OK;
        case DML_KNOB_INDEX_CUS: return set_cu_split(s, (int)(value & 0xFFFF), (int)(value >> 16));
        case DML_KNOB_FETCH_KERNEL:
            if ((value & 0xFF) > 2 || (value >> 8) >= kFetchVariants)
                return set_err(DML_E_INVALID_ARG, "bad fetch kernel choice");
            s->fetch_kernel = value;
            return DML_OK;
        default: return set_err(DML_E_INVALID_ARG, "unknown knob");
    }
}

// launch_chunk's plan for an array chunk, by the functions launch_chunk and
// launch_sparse_leaf call, in their order; nothing here touches a device.
int dml_diag_sparse_plan(int32_t value_type, int64_t rows, const int64_t* nrecs, int32_t n, int32_t tail_cut,
                         dml_sparse_plan_info* out) {
    if (!nrecs || !out || n < 1 || n > kMaxW || rows < 1 || rows > INT32_MAX ||
        (value_type != kI32 && value_type != kF32 && value_type != kF64))
        return set_err(DML_E_INVALID_ARG, "bad sparse plan arguments");
    Batch bt{};
    for (int b = 0; b < n; ++b) {
        if (nrecs[b] < 0) return set_err(DML_E_INVALID_ARG, "negative record count");
        bt.nrec[b] = nrecs[b];
    }
    SpPlan pl = sparse_plan(bt, n, rows);
    pl.compact = sparse_compact_ok(value_type, pl, tail_cut != 0);
    sparse_plan_big(pl, bt, rows);
    *out = dml_sparse_plan_info{};
    out->nrec = pl.nrec;
    out->nleaves = pl.nleaves;
    out->cap1 = pl.cap1;
    out->cap2 = pl.cap2;
    out->SL = pl.SL;
    out->D2 = pl.D2;
    out->nbins1 = pl.nbins1;
    out->compact = pl.compact;
    out->big = pl.big;
    if (pl.big) {
        out->BL = pl.BL;
        out->nbig = pl.nbig;
        out->capS = pl.capS;
    }
    out->bshift = pl.big ? sparse_big_bshift(pl.BL) : sparse_leaf_bshift(pl.SL);
    return DML_OK;
}

int dml_store_kernel_name(dml_store* s, char* out, int32_t cap) {
    if (int rc = check_store(s)) return rc;
    if (!out || cap <= 0) return set_err(DML_E_INVALID_ARG, "bad name buffer");
    std::lock_guard<std::mutex> lk(s->mu);
    const char* n = s->kname ? s->kname : "";
    std::snprintf(out, (size_t)cap, "%s", n);
    return (int32_t)std::strlen(n) < cap ? DML_OK : set_err(DML_E_CAPACITY, "name buffer too small");
}

int dml_store_kernel_time(dml_store* s, double* total_ms, int64_t* launches, int32_t reset) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    ev_collect(s);
    if (total_ms) *total_ms = s->timed_ms;
    if (launches) *launches = s->timed_n;
    if (reset) {
        s->timed_ms = 0.0;
        s->timed_n = 0;
    }
    return DML_OK;
}

// ---- synthetic data --------------------------------------------------------
int dml_synth_dense_bucket(void* dev_out, const dml_desc* desc, int64_t first_key, int64_t shard_rows, int64_t nrec,
                           int32_t cols, uint64_t seed, uint64_t perm_a, uint64_t perm_c, void* stream) {
    if (!dev_out || !desc || shard_rows <= 0 || nrec < 0 || cols <= 0) return set_err(DML_E_INVALID_ARG, "bad synth args");
    if (perm_a >= (1ull << 32) || (uint64_t)nrec >= (1ull << 32)) return set_err(DML_E_INVALID_ARG, "perm_a/nrec must be < 2^32");
    const int K = desc_key_bytes(*desc);
    HIPCHK(launch_synth_dense((uint8_t*)dev_out, K, desc->value_type, first_key, shard_rows, nrec, cols,
                              splitmix64(seed), perm_a % (uint64_t)shard_rows, perm_c % (uint64_t)shard_rows,
                              (hipStream_t)stream));
    return DML_OK;
}

int dml_synth_sparse_bucket(void* dev_out, const dml_desc* desc, int64_t first_key, int64_t key_space, int64_t nrec,
                            uint64_t seed, uint64_t perm_a, uint64_t perm_c, void* stream) {
    if (!dev_out || !desc || key_space <= 0 || nrec < 0) return set_err(DML_E_INVALID_ARG, "bad synth args");
    if (perm_a >= (1ull << 32) || (uint64_t)nrec >= (1ull << 32)) return set_err(DML_E_INVALID_ARG, "perm_a/nrec must be < 2^32");
    const int K = desc_key_bytes(*desc);
    const int V = desc_value_bytes(*desc);
    HIPCHK(launch_synth_sparse((uint8_t*)dev_out, K, desc->value_type, V, first_key, key_space, nrec, splitmix64(seed),
                               perm_a % (uint64_t)key_space, perm_c % (uint64_t)key_space, (hipStream_t)stream));
    return DML_OK;
}

int dml_diag_stream(int32_t copy, void* dev_dst, const void* dev_src, int64_t bytes, void* stream, float* ms) {
    if (!dev_dst || !dev_src || bytes < 0 || bytes % 16 || ((uintptr_t)dev_dst | (uintptr_t)dev_src) % 16)
        return set_err(DML_E_INVALID_ARG, "stream copy needs 16-B aligned buffers and a multiple of 16 bytes");
    return timed_launch(ms, [&](LaunchEv ev) {
        return launch_stream(copy != 0, dev_dst, dev_src, bytes / 16, (hipStream_t)stream, ev);
    });
}

int dml_diag_ring_rs(int32_t value_type, const void* dev_partial, void* dev_recv, void* dev_landing,
                     int64_t chunk_bytes, int32_t world, int32_t rank, int32_t channels, void* stream) {
    if (!dev_partial || !dev_recv || !dev_landing || chunk_bytes < 0 || chunk_bytes % 16 || world < 1 || rank < 0 ||
        rank >= world || channels < 1)
        return set_err(DML_E_INVALID_ARG, "bad ring reduce-scatter arguments");
    HIPCHK(launch_ring_rs(value_type, dev_partial, dev_recv, dev_landing, chunk_bytes, world, rank, channels,
                          (hipStream_t)stream));
    return DML_OK;
}

int dml_diag_rmw_floor(float* dev_array, const uint32_t* dev_index, const float* dev_values, int64_t n, void* stream,
                       float* ms) {
    if (!dev_array || n < 0 || (n > 0 && (!dev_index || !dev_values)))
        return set_err(DML_E_INVALID_ARG, "bad rmw floor arguments");
    return timed_launch(ms, [&](LaunchEv ev) {
        return launch_rmw_floor(dev_array, dev_index, dev_values, n, (hipStream_t)stream, ev);
    });
}

int dml_diag_dense_floor(dml_store* s, const void* const* dev_bufs, const int64_t* lens, int32_t n, void* stream,
                         float* ms, int32_t* out_of_place) {
    if (int rc = check_store(s)) return rc;
    if (!s->is_matrix || s->V != 4 || vtype_of(s->desc) != kF32 || s->cols % 4 || n < 1 || n > kMaxW || !dev_bufs ||
        !lens)
        return set_err(DML_E_INVALID_ARG, "dense floor: an f32 matrix store of whole 16-B vectors, 1..64 pushes");
    for (int b = 0; b < n; ++b)
        if (!dev_bufs[b] || lens[b] != s->rows * s->stride)
            return set_err(DML_E_INVALID_ARG, "dense floor: every push lists every row once (full range)");
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    Batch bt{};
    for (int b = 0; b < n; ++b) bt.base[b] = (const uint8_t*)dev_bufs[b];
    // out of place into the speculative second buffer where the store has one (k_flat_ident's
    // layout); AdaGrad stores apply in place (k_ada_ident)
    float* out = (float*)(s->data_alt && !s->adagrad ? s->data_alt : s->data);
    if (out_of_place) *out_of_place = out != s->data ? 1 : 0;
    return timed_launch(ms, [&](LaunchEv ev) {
        return launch_dense_floor((const float*)s->data, out, s->adagrad ? s->delta : nullptr, bt, n, s->stride, s->K,
                                  s->cols, s->rows * s->cols, (hipStream_t)stream, ev);
    });
}

int dml_diag_gather_floor(int32_t* dev_shard, int32_t cols, const int32_t* dev_rows, const int32_t* dev_ptr,
                          const uint64_t* dev_addr, int64_t ntouched, void* stream, float* ms) {
    if (!dev_shard || cols <= 0 || cols % 4 || cols > 1024 || ntouched < 0 ||
        (ntouched > 0 && (!dev_rows || !dev_ptr || !dev_addr)) || (uintptr_t)dev_shard % 16)
        return set_err(DML_E_INVALID_ARG, "bad gather floor arguments (cols a multiple of 4, at most 1024)");
    return timed_launch(ms, [&](LaunchEv ev) {
        return launch_gather_floor(dev_shard, cols, dev_rows, dev_ptr, dev_addr, ntouched, (hipStream_t)stream, ev);
    });
}

int dml_store_rand(dml_store* s, uint64_t seed) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    const int vt = vtype_of(s->desc);
    if (!s->is_matrix || vt == kI32) return DML_OK;  // DataStore.rand(): no-op (DataStore.java:22)
    if (vt == kF64) {
        // DoubleMatrixStore.rand() seeds Random(1L) on every shard: reproduced exactly,
        // on the host (init, not the push path), a block of rows at a time
        const int64_t cols = s->cols, rb = std::max<int64_t>(1, (int64_t(1) << 21) / cols);
        JavaRandom jr(1);
        std::vector<double> blk((size_t)(std::min(rb, s->rows) * cols));
        for (int64_t r0 = 0; r0 < s->rows; r0 += rb) {
            const int64_t nr = std::min(rb, s->rows - r0);
            for (int64_t i = 0; i < nr; ++i) java_unit_abs_gaussian_row(jr, blk.data() + i * cols, cols);
            HIPCHK(hipMemcpyAsync((double*)s->data + r0 * cols, blk.data(), (size_t)(nr * cols) * 8,
                                  hipMemcpyHostToDevice, s->stream));
            HIPCHK(hipStreamSynchronize(s->stream));
        }
        return DML_OK;
    }
    HIPCHK(launch_rand(vt, s->data, s->rows, s->cols, splitmix64(seed ^ 0x5241'4e44ull), s->stream));
    return drain(s);
}

int dml_synth_fill_store(dml_store* s, uint64_t seed) {
    if (int rc = check_store(s)) return rc;
    Entry in(s);
    if (int rc = begin_call(s)) return rc;
    HIPCHK(launch_synth_fill(vtype_of(s->desc), s->data, s->rows * s->cols, splitmix64(seed), s->stream));
    return drain(s);
}

}  // extern "C"

// dml_codec.hip — the device record codec (C-ABI dml_records_pack_device,
// dml_records_unpack_device, dml_record_bytes).
//
// The client side of a push writes its rows as wire records (SparseMatrix.writeMap dense
// branch, SparseMatrix.java:96-148; SparseArray.writeMap, SparseArray.java:63-76) and reads
// a fetch's records back into rows (the matching readMap). These calls are that pair for a
// worker whose tensors are in HBM: pack turns a dense T[n][cols] buffer plus keys into the
// push layout dml_store_push_batch_device and the dml_group_push_* calls read; unpack turns
// the handleFetch layout dml_store_fetch_device and dml_group_pull write into a dense
// values plane, AdaGrad's alpha plane and an int64 key plane. Store-less, like
// dml_shard_split: a dml_desc describes the layout.
//
// Both kernels are output-stationary in k_fetch_vec's shape (§4.10): the output is cut at
// the 16-byte lines of its ADDRESS (4-byte aligned only: `lead` dwords of the first line
// lie before it), one thread owns one line, 256 lines per block, blocks in dispatch order;
// one division per line finds its record or row; a line leaves as one non-temporal 16-byte
// store, single dwords only on a plane's first and last line. Every move is a dword move:
// no float instruction touches a value. No LDS, no scratch.
//   k_rec_pack     fetch_line (dml_fetch_line.h) with record j's row = row j of the values
//                  buffer: no key is refused, so no `bad` word and no verdict kernel
//   k_rec_unpack   one plane: element e of T[n][cols] is row j = e / rowdw, column c, read
//                  from record dword j x recdw + kdw + c x stride + component (stride 2 for
//                  AdaGrad's [value][alpha] pairs and FloatArrayStore's [value][pad] slot)
//   k_rec_keys     one thread per record: the key, sign-extended (ld_key), as one int64
#include <atomic>

#include "distml_ps.h"
#include "dml_fetch_line.h"
#include "dml_host.h"

using namespace dml;

namespace {

constexpr int kCodecBlock = 256;  // lines per block: DML_CODEC_BLOCK_BYTES / 16
static_assert(kCodecBlock * 16 == DML_CODEC_BLOCK_BYTES && 64 * 16 == DML_CODEC_WAVE_BYTES, "exported tile sizes");

template <int LAYOUT, bool VLOAD, bool WIDE>
__global__ __launch_bounds__(kCodecBlock) void k_rec_pack(const FetchP a, int64_t nline) {
    const int64_t v = (int64_t)blockIdx.x * kCodecBlock + threadIdx.x;
    if (v < nline) fetch_line<LAYOUT, VLOAD, kRowOfRecord, WIDE>(a, v);
}

struct UnpackP {
    const uint32_t* rec;  // the records, as dwords
    uint8_t* line0;       // the plane rounded down to 16 bytes
    int64_t ndw;          // dwords of the plane (n x rowdw)
    int32_t rowdw;        // dwords of one row of the plane
    int32_t recdw, kdw;   // dwords of one record, and of its key
    int32_t comp;         // STRIDE 2: 0 = the slot's first dword (value), 1 = its second (alpha)
    int32_t lead;
};

// STRIDE: source dwords per plane dword (1: plain layouts; 2: AdaGrad pairs, FloatArrayStore slots).
// VLOAD: a line inside one row is one 4-byte-aligned 16-byte load (STRIDE 1) or two, with the
// component picked in registers (STRIDE 2); every other line gathers its dwords singly.
template <int STRIDE, bool VLOAD, bool WIDE>
__global__ __launch_bounds__(kCodecBlock) void k_rec_unpack(const UnpackP a, int64_t nline) {
    const int64_t v = (int64_t)blockIdx.x * kCodecBlock + threadIdx.x;
    if (v >= nline) return;
    const int64_t d0 = 4 * v - a.lead;  // plane dword of the line's first slot (< 0 only on line 0)
    const int64_t lo = d0 < 0 ? 0 : d0;
    const int64_t hi = d0 + 4 < a.ndw ? d0 + 4 : a.ndw;
    if (lo >= hi) return;
    int64_t j;
    // narrowed: lo < ndw <= 2^32 - 1 and rowdw < 2^31, so both fit a uint32
    if (!WIDE && a.ndw <= 0xFFFFFFFFll) j = (int64_t)((uint32_t)lo / (uint32_t)a.rowdw);
    else j = lo / a.rowdw;
    int32_t c = (int32_t)(lo - j * a.rowdw);  // dword inside row j
    const uint32_t* src = a.rec + j * a.recdw + a.kdw;  // record j's first slot
    uint8_t* o = a.line0 + 16 * v;
    if (VLOAD && hi - lo == 4 && c + 4 <= a.rowdw) {
        if (STRIDE == 1) {
            stg16_nt(o, ldg16((const uint8_t*)(src + c)));
        } else {  // slots c .. c + 3: eight dwords, all inside record j
            const u32x4 x = ldg16((const uint8_t*)(src + 2 * c)), y = ldg16((const uint8_t*)(src + 2 * c + 4));
            u32x4 q;
            q.x = a.comp ? x.y : x.x; q.y = a.comp ? x.w : x.z; q.z = a.comp ? y.y : y.x; q.w = a.comp ? y.w : y.z;
            stg16_nt(o, q);
        }
        return;
    }
    uint32_t val[4] = {0u, 0u, 0u, 0u};
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t d = d0 + e;
        if (d < lo || d >= hi) continue;
        if (c == a.rowdw) {
            c = 0;
            src += a.recdw;
        }
        val[e] = ldg32((const uint8_t*)(src + STRIDE * c + (STRIDE == 2 ? a.comp : 0)));
        mask |= 1u << e;
        ++c;
    }
    if (mask == 0xFu) {
        u32x4 q;
        q.x = val[0]; q.y = val[1]; q.z = val[2]; q.w = val[3];
        stg16_nt(o, q);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (mask & (1u << e)) stg32_nt(o + 4 * e, val[e]);
    }
}

__global__ __launch_bounds__(kCodecBlock) void k_rec_keys(const uint8_t* rec, int64_t n, int64_t rec_bytes, int K,
                                                         int64_t* out) {
    const int64_t j = (int64_t)blockIdx.x * kCodecBlock + threadIdx.x;
    if (j < n) out[j] = ld_key(rec + j * rec_bytes, K);
}

// Records of at least this many dwords take the 16-byte loads; shorter ones gather every
// dword singly. Each from this kernel's own rounds (scripts/ubench_codec.py).
// Pack: 65-dword records run 6-8 % faster gathered (17-dword ones 2.2 x), 97-dword ones tie
// (0.5 % and 3 % for the loads in two runs), 129- to 1 025-dword ones run 2-9 % faster with
// the loads; the threshold sits between the measured neighbours 65 and 97.
constexpr int32_t kPackVloadMinDw = 80;
// Unpack, plain layouts: the gathers won or tied at every length measured from 65 to 1 025
// dwords (5-9 % at config 4's 201), so no length takes the loads; the knob still runs them.
constexpr int32_t kUnpackVloadMinDw = 0x7FFFFFFF;
// Unpack, AdaGrad's pairs: the two 16-byte loads won at every length measured, from the
// shortest (17 dwords, 4 %) to 401 (12 %) and 1 025 (10 %); shorter records are unmeasured and gather.
constexpr int32_t kUnpackPairVloadMinDw = 17;

// dml_diag_codec_knob: process-wide, read at every launch
std::atomic<int> g_wide{0};   // 1: 64-bit line division on every stream
std::atomic<int> g_loads{0};  // 0: by record length, 1: every dword singly, 2: 16-byte loads

bool pick_vload(int32_t recdw, int32_t min_dw) {
    const int mode = g_loads.load();
    return mode == 2 || (mode == 0 && recdw >= min_dw);
}

// The layouts of a desc: key and value bytes, columns, the push and fetch record bytes.
struct Layout {
    int K, V;
    int32_t cols;  // 1 for arrays
    bool ada;      // FloatMatrixStoreAdaGrad: the fetch interleaves [value][alpha]
    bool slot8;    // FloatArrayStore: the fetch's 8-byte slot
    bool pad_push; // ... and the push's, under DML_FLAG_FLOAT_ARRAY_REF_STRIDE
    int64_t push_rec, fetch_rec;
};

constexpr uint32_t kKnownFlags = DML_FLAG_FLOAT_ARRAY_REF_STRIDE | DML_FLAG_ASYNC | DML_FLAG_NO_SPECULATION;

int layout_of(const dml_desc* desc, int32_t cols, uint32_t flags, Layout* l) {
    if (!desc) return set_error(DML_E_INVALID_ARG, "null desc");
    const dml_desc d = *desc;
    if ((d.data_type != 0 && d.data_type != 1) || (d.key_type != 0 && d.key_type != 1) ||
        (d.value_type != DML_ELEMENT_TYPE_INT && d.value_type != DML_ELEMENT_TYPE_FLOAT &&
         d.value_type != DML_ELEMENT_TYPE_DOUBLE))
        return set_error(DML_E_BAD_DESC, "Unrecognized matrix type (DataStore.createStore)");
    if (flags & ~kKnownFlags) return set_error(DML_E_INVALID_ARG, "unknown flag bit");
    const bool matrix = d.data_type == DML_DATA_TYPE_MATRIX;
    if (matrix && !d.dense_column)
        return set_error(DML_E_UNSUPPORTED, "sparse-column matrix records are not supported (SURVEY defect 3)");
    if (matrix && cols <= 0) return set_error(DML_E_INVALID_ARG, "cols must be > 0");
    l->K = desc_key_bytes(d);
    l->V = desc_value_bytes(d);
    l->cols = matrix ? cols : 1;
    const bool f32 = d.value_type == DML_ELEMENT_TYPE_FLOAT;
    l->ada = matrix && f32 && d.ada_grad;
    l->slot8 = !matrix && f32;
    l->pad_push = l->slot8 && (flags & DML_FLAG_FLOAT_ARRAY_REF_STRIDE);
    l->push_rec = l->K + (l->pad_push ? 8 : (int64_t)l->V * l->cols);
    l->fetch_rec = l->K + (l->ada || l->slot8 ? (int64_t)8 * l->cols : (int64_t)l->V * l->cols);
    // the kernels hold a record's dword count and a dword's place in it as int32
    if (l->fetch_rec / 4 > 0x7FFFFFFF) return set_error(DML_E_UNSUPPORTED, "records of 2^31 dwords and more");
    return DML_OK;
}

bool overlap(const void* a, int64_t alen, const void* b, int64_t blen) {
    if (!a || !b || alen <= 0 || blen <= 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)blen && y < x + (uintptr_t)alen;
}

template <int LAYOUT>
void launch_pack(const FetchP& a, int64_t nline, hipStream_t st) {
    const dim3 grid((unsigned)((nline + kCodecBlock - 1) / kCodecBlock)), blk(kCodecBlock);
    const bool vload = LAYOUT == kPlain && pick_vload(a.recdw, kPackVloadMinDw);
    switch ((vload ? 1 : 0) | (g_wide.load() ? 2 : 0)) {
        case 0: hipLaunchKernelGGL((k_rec_pack<LAYOUT, false, false>), grid, blk, 0, st, a, nline); break;
        case 1: hipLaunchKernelGGL((k_rec_pack<LAYOUT, true, false>), grid, blk, 0, st, a, nline); break;
        case 2: hipLaunchKernelGGL((k_rec_pack<LAYOUT, false, true>), grid, blk, 0, st, a, nline); break;
        default: hipLaunchKernelGGL((k_rec_pack<LAYOUT, true, true>), grid, blk, 0, st, a, nline); break;
    }
}

template <int STRIDE>
void launch_unpack(const UnpackP& a, int64_t nline, hipStream_t st) {
    const dim3 grid((unsigned)((nline + kCodecBlock - 1) / kCodecBlock)), blk(kCodecBlock);
    const bool vload = pick_vload(a.recdw, STRIDE == 1 ? kUnpackVloadMinDw : kUnpackPairVloadMinDw);
    switch ((vload ? 1 : 0) | (g_wide.load() ? 2 : 0)) {
        case 0: hipLaunchKernelGGL((k_rec_unpack<STRIDE, false, false>), grid, blk, 0, st, a, nline); break;
        case 1: hipLaunchKernelGGL((k_rec_unpack<STRIDE, true, false>), grid, blk, 0, st, a, nline); break;
        case 2: hipLaunchKernelGGL((k_rec_unpack<STRIDE, false, true>), grid, blk, 0, st, a, nline); break;
        default: hipLaunchKernelGGL((k_rec_unpack<STRIDE, true, true>), grid, blk, 0, st, a, nline); break;
    }
}

// One plane of n x rowdw dwords at `plane` (4-byte aligned), component `comp` of each slot.
void unpack_plane(const Layout& l, const void* records, int64_t n, void* plane, int comp, hipStream_t st) {
    const int stride = l.ada || l.slot8 ? 2 : 1;
    UnpackP a;
    a.rec = (const uint32_t*)records;
    a.lead = (int32_t)(((uintptr_t)plane & 15) >> 2);
    a.line0 = (uint8_t*)plane - 4 * a.lead;
    a.rowdw = (int32_t)((int64_t)l.cols * (stride == 2 ? 4 : l.V) / 4);
    a.ndw = n * a.rowdw;
    a.recdw = (int32_t)(l.fetch_rec / 4);
    a.kdw = l.K / 4;
    a.comp = comp;
    const int64_t nline = (a.ndw + a.lead + 3) / 4;
    if (stride == 2) launch_unpack<2>(a, nline, st);
    else launch_unpack<1>(a, nline, st);
}

}  // namespace

extern "C" int dml_record_bytes(const dml_desc* desc, int32_t cols, uint32_t flags, int64_t* push_rec,
                                int64_t* fetch_rec) {
    Layout l;
    if (int rc = layout_of(desc, cols, flags, &l)) return rc;
    if (push_rec) *push_rec = l.push_rec;
    if (fetch_rec) *fetch_rec = l.fetch_rec;
    return DML_OK;
}

extern "C" int dml_records_pack_device(const dml_desc* desc, int32_t cols, uint32_t flags, const int64_t* dev_keys,
                                       int64_t key_lo, int64_t n, const void* dev_values, void* dev_out, int64_t cap,
                                       int64_t* out_len, void* stream) {
    if (!out_len) return set_error(DML_E_INVALID_ARG, "null out_len");
    *out_len = 0;
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative record count");
    Layout l;
    if (int rc = layout_of(desc, cols, flags, &l)) return rc;
    if (n > INT64_MAX / l.push_rec) return set_error(DML_E_INVALID_ARG, "record count overflows the byte length");
    *out_len = n * l.push_rec;
    if (((uintptr_t)dev_keys & 7u) != 0) return set_error(DML_E_INVALID_ARG, "keys are not 8-byte aligned");
    if ((((uintptr_t)dev_values | (uintptr_t)dev_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "values or output pointer is not 4-byte aligned");
    if (n == 0) return DML_OK;
    if (!dev_values || !dev_out) return set_error(DML_E_INVALID_ARG, "null values or output pointer");
    if (cap < *out_len) return set_error(DML_E_CAPACITY, "pack output buffer too small");
    const int64_t vbytes = n * l.cols * l.V;
    if (overlap(dev_out, *out_len, dev_values, vbytes) || overlap(dev_out, *out_len, dev_keys, n * 8))
        return set_error(DML_E_INVALID_ARG, "pack output overlaps an input");
    FetchP a;
    a.data = (const uint32_t*)dev_values;
    a.alpha = nullptr;
    a.keys = dev_keys;
    a.key_lo = key_lo;
    a.first = a.last = 0;
    a.lead = (int32_t)(((uintptr_t)dev_out & 15) >> 2);
    a.line0 = (uint8_t*)dev_out - 4 * a.lead;
    a.recdw = (int32_t)(l.push_rec / 4);
    a.ndw = n * a.recdw;
    a.rowdw = (int64_t)l.cols * (l.V / 4);
    a.cols = l.cols;
    a.kdw = l.K / 4;
    a.bad = nullptr;
    const int64_t nline = (a.ndw + a.lead + 3) / 4;
    hipStream_t st = (hipStream_t)stream;
    if (l.pad_push) launch_pack<kPad>(a, nline, st);
    else launch_pack<kPlain>(a, nline, st);
    HIPCHK(hipGetLastError());
    if (!st) HIPCHK(hipStreamSynchronize(st));
    return DML_OK;
}

extern "C" int dml_records_unpack_device(const dml_desc* desc, int32_t cols, uint32_t flags, const void* dev_records,
                                         int64_t n, int64_t* dev_keys_out, void* dev_values_out, float* dev_alpha_out,
                                         void* stream) {
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative record count");
    Layout l;
    if (int rc = layout_of(desc, cols, flags, &l)) return rc;
    if (n > INT64_MAX / l.fetch_rec) return set_error(DML_E_INVALID_ARG, "record count overflows the byte length");
    if (!dev_keys_out && !dev_values_out && !dev_alpha_out) return set_error(DML_E_INVALID_ARG, "no output plane");
    if (dev_alpha_out && !l.ada) return set_error(DML_E_INVALID_ARG, "an alpha plane, but not an AdaGrad desc");
    if (((uintptr_t)dev_keys_out & 7u) != 0) return set_error(DML_E_INVALID_ARG, "key plane is not 8-byte aligned");
    if ((((uintptr_t)dev_records | (uintptr_t)dev_values_out | (uintptr_t)dev_alpha_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "records or plane pointer is not 4-byte aligned");
    if (n == 0) return DML_OK;
    if (!dev_records) return set_error(DML_E_INVALID_ARG, "null records pointer");
    const int64_t rbytes = n * l.fetch_rec, vbytes = n * l.cols * l.V, abytes = n * l.cols * 4, kbytes = n * 8;
    if (overlap(dev_values_out, vbytes, dev_records, rbytes) || overlap(dev_alpha_out, abytes, dev_records, rbytes) ||
        overlap(dev_keys_out, kbytes, dev_records, rbytes))
        return set_error(DML_E_INVALID_ARG, "unpack output overlaps the records");
    if (overlap(dev_values_out, vbytes, dev_alpha_out, abytes) || overlap(dev_values_out, vbytes, dev_keys_out, kbytes) ||
        overlap(dev_alpha_out, abytes, dev_keys_out, kbytes))
        return set_error(DML_E_INVALID_ARG, "unpack output planes overlap");
    hipStream_t st = (hipStream_t)stream;
    if (dev_values_out) unpack_plane(l, dev_records, n, dev_values_out, 0, st);
    if (dev_alpha_out) unpack_plane(l, dev_records, n, dev_alpha_out, 1, st);
    if (dev_keys_out)
        hipLaunchKernelGGL(k_rec_keys, dim3((unsigned)((n + kCodecBlock - 1) / kCodecBlock)), dim3(kCodecBlock), 0, st,
                           (const uint8_t*)dev_records, n, l.fetch_rec, l.K, dev_keys_out);
    HIPCHK(hipGetLastError());
    if (!st) HIPCHK(hipStreamSynchronize(st));
    return DML_OK;
}

extern "C" int dml_diag_codec_knob(int32_t knob, int64_t value) {
    if (knob == DML_CODEC_KNOB_WIDE_INDEX && (value == 0 || value == 1)) {
        g_wide.store((int)value);
        return DML_OK;
    }
    if (knob == DML_CODEC_KNOB_LOADS && value >= 0 && value <= 2) {
        g_loads.store((int)value);
        return DML_OK;
    }
    return set_error(DML_E_INVALID_ARG, "unknown codec knob or value");
}

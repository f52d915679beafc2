// dml_fetch.hip — the record encode of dml_store_fetch_device.
//
// handleFetch's dense-column layouts (FloatMatrixStore.java:113-174,
// IntMatrixStore.java:81-140, DoubleMatrixStore.java:80-139,
// FloatMatrixStoreAdaGrad.java:146-213, FloatArrayStore.java:88-108,
// IntArrayStore.java:78-95, DoubleArrayStore.java:93-113) as ONE packed stream of
// nkeys records, written in whole 16-byte vectors.
//
// k_fetch_vec is output-stationary. The stream is cut at the 16-byte lines of the
// output ADDRESS (dev_out is 4-byte aligned only: `lead` dwords of the first line lie
// before it), and one thread owns one such line: it finds the record its first dword
// falls in (one division per line, 32-bit when the stream is under 2^32 dwords), then
// walks its four dwords through at most three records. With records of kFetchVloadMinDw
// dwords or more, a line inside one record's values of a plain store is one
// 4-byte-aligned 16-byte load of the shard, and AdaGrad's [value][alpha] pairs are two
// 8-byte loads interleaved in registers; every other line (one with a key, a record
// boundary, FloatArrayStore's zero pad, and every line of shorter records) gathers its
// dwords singly. All four dwords leave in one non-temporal 16-byte store; only the
// stream's first and last line, and a line that touches a refused record, fall back
// to single dwords. Bytes pass through as uint32: no float instruction touches them.
//
// A key is loaded once per record a line touches (the range form computes it). A key
// outside [first, last] is never turned into an address: its record's dwords are
// skipped, and the thread that owns the record's first dword reports the list index.
#include "dml_device.h"

namespace dml {

namespace {

constexpr int kPlain = 0;  // values are the shard's dwords in order (f32, i32, f64 matrices and arrays)
constexpr int kAda = 1;    // [value][alpha] pairs (FloatMatrixStoreAdaGrad)
constexpr int kPad = 2;    // [value][0] (FloatArrayStore's 8-byte slot)

struct FetchP {
    const uint32_t* data;   // the shard, as dwords
    const uint32_t* alpha;  // kAda
    const int64_t* keys;    // null: key = key_lo + record index
    int64_t key_lo, first, last;
    uint8_t* line0;         // dev_out rounded down to 16 bytes
    int64_t ndw;            // dwords of the stream
    int64_t rowdw;          // dwords of one shard row (cols x V / 4)
    int32_t cols, recdw, kdw, lead;
    unsigned long long* bad;
};

__device__ inline void stg32_nt(void* p, uint32_t v) { __builtin_nontemporal_store(v, (DML_GLOBAL uint32_t*)p); }
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_u __attribute__((aligned(4)));
__device__ inline u32x2 ldg8(const uint32_t* p) { return *(const DML_GLOBAL u32x2_u*)p; }

template <int LAYOUT, bool VLOAD>
__device__ inline void fetch_line(const FetchP& a, int64_t v) {
    const int64_t d0 = 4 * v - a.lead;  // stream dword of the line's first slot (< 0 only on line 0)
    const int64_t lo = d0 < 0 ? 0 : d0;
    const int64_t hi = d0 + 4 < a.ndw ? d0 + 4 : a.ndw;
    if (lo >= hi) return;
    int64_t j;
    if (a.ndw <= 0xFFFFFFFFll) j = (int64_t)((uint32_t)lo / (uint32_t)a.recdw);
    else j = lo / a.recdw;
    int32_t w = (int32_t)(lo - j * a.recdw);  // dword inside record j

    int64_t key = a.keys ? a.keys[j] : a.key_lo + j;
    bool good = key >= a.first && key <= a.last;
    int64_t idx = key - a.first;

    if (good && w >= a.kdw && w + 4 <= a.recdw && hi - lo == 4) {
        const int32_t c = w - a.kdw;
        if (LAYOUT == kPlain && VLOAD) {
            stg16_nt(a.line0 + 16 * v, ldg16((const uint8_t*)(a.data + idx * a.rowdw + c)));
            return;
        }
        if (LAYOUT == kAda && VLOAD && (c & 1) == 0) {
            const int64_t e = idx * a.cols + (c >> 1);
            const u32x2 x = ldg8(a.data + e), al = ldg8(a.alpha + e);
            u32x4 o;
            o.x = x.x; o.y = al.x; o.z = x.y; o.w = al.y;
            stg16_nt(a.line0 + 16 * v, o);
            return;
        }
    }

    uint32_t val[4] = {0u, 0u, 0u, 0u};
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t d = d0 + e;
        if (d < lo || d >= hi) continue;
        if (w == a.recdw) {
            w = 0;
            ++j;
            key = a.keys ? a.keys[j] : a.key_lo + j;
            good = key >= a.first && key <= a.last;
            idx = key - a.first;
        }
        if (!good) {
            if (w == 0) atomicMin(a.bad, (unsigned long long)j);
        } else {
            uint32_t x;
            if (w < a.kdw) {
                x = w == 0 ? (uint32_t)key : (uint32_t)((uint64_t)key >> 32);
            } else {
                const int32_t c = w - a.kdw;
                if (LAYOUT == kPlain) x = a.data[idx * a.rowdw + c];
                else if (LAYOUT == kAda) x = (c & 1) ? a.alpha[idx * a.cols + (c >> 1)] : a.data[idx * a.cols + (c >> 1)];
                else x = (c & 1) ? 0u : a.data[idx];
            }
            val[e] = x;
            mask |= 1u << e;
        }
        ++w;
    }
    uint8_t* o = a.line0 + 16 * v;
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

// U lines per thread, a block's U x 256 lines contiguous, one wave instruction's 64 lines
// contiguous (DML_FETCH_WAVE_BYTES; DML_FETCH_BLOCK_BYTES is the shipped U = 1). Blocks run
// in dispatch order: xcd_block() numbering measured 1.5-3 % slower here.
template <int LAYOUT, bool VLOAD, bool XCD, int U>
__global__ __launch_bounds__(256) void k_fetch_vec(const FetchP a, int64_t nline) {
    const int64_t blk = XCD ? xcd_block() : (int64_t)blockIdx.x;
    const int64_t v0 = blk * (256 * U) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * 256;
        if (v < nline) fetch_line<LAYOUT, VLOAD>(a, v);
    }
}

__global__ void k_fetch_verdict(unsigned long long* bad, const int64_t* keys, FetchVerdict* v) {
    const unsigned long long i = *bad;
    if (i == kNoPos) return;
    if (v->idx == kNoPos) {
        v->key = keys[i];
        v->idx = i;
    }
    *bad = kNoPos;
}

template <int LAYOUT, bool VLOAD, bool XCD, int U>
void launch_t(const FetchP& a, int64_t nline, hipStream_t st) {
    const int64_t per = 256 * U;
    hipLaunchKernelGGL((k_fetch_vec<LAYOUT, VLOAD, XCD, U>), dim3((unsigned)((nline + per - 1) / per)), dim3(256), 0, st,
                       a, nline);
}
// Records of at least this many dwords take the 16-byte shard loads; shorter ones gather
// every dword singly (with a record boundary in every wave both paths of
// the load run in every wave, and the single path is the faster one).
constexpr int32_t kFetchVloadMinDw = 768;
constexpr bool kFetchOnePerThread = true;   // the shipped lines per thread: 1, or 4

template <int LAYOUT>
void launch_l(const FetchP& a, int64_t nline, int variant, hipStream_t st) {
    const int mode = variant & kFetchVarLoadMask;
    const bool vload = mode == kFetchVarVload || (mode == 0 && a.recdw >= kFetchVloadMinDw);
    const bool xcd = (variant & kFetchVarXcd) != 0;
    const bool u1 = (variant & kFetchVarU1) != 0 || (kFetchOnePerThread && (variant & kFetchVarU4) == 0);
    switch ((vload ? 1 : 0) | (xcd ? 2 : 0) | (u1 ? 4 : 0)) {
        case 0: return launch_t<LAYOUT, false, false, 4>(a, nline, st);
        case 1: return launch_t<LAYOUT, true, false, 4>(a, nline, st);
        case 2: return launch_t<LAYOUT, false, true, 4>(a, nline, st);
        case 3: return launch_t<LAYOUT, true, true, 4>(a, nline, st);
        case 4: return launch_t<LAYOUT, false, false, 1>(a, nline, st);
        case 5: return launch_t<LAYOUT, true, false, 1>(a, nline, st);
        case 6: return launch_t<LAYOUT, false, true, 1>(a, nline, st);
        default: return launch_t<LAYOUT, true, true, 1>(a, nline, st);
    }
}

}  // namespace

hipError_t launch_fetch_vec(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                            int64_t key_lo, int64_t n, int64_t first, int64_t last, uint8_t* out, int64_t rec, int K,
                            int value_slot, unsigned long long* bad, int variant, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int V = vtype == kF64 ? 8 : 4;
    FetchP a;
    a.data = (const uint32_t*)shard;
    a.alpha = (const uint32_t*)alpha;
    a.keys = keys;
    a.key_lo = key_lo;
    a.first = first;
    a.last = last;
    a.lead = (int32_t)(((uintptr_t)out & 15) >> 2);
    a.line0 = out - 4 * a.lead;
    a.ndw = n * (rec / 4);
    a.rowdw = (int64_t)cols * (V / 4);
    a.cols = cols;
    a.recdw = (int32_t)(rec / 4);
    a.kdw = K / 4;
    a.bad = bad;
    const int64_t nline = (a.ndw + a.lead + 3) / 4;
    if (alpha) launch_l<kAda>(a, nline, variant, st);
    else if (value_slot != V) launch_l<kPad>(a, nline, variant, st);
    else launch_l<kPlain>(a, nline, variant, st);
    return hipGetLastError();
}

hipError_t launch_fetch_verdict(unsigned long long* bad, const int64_t* keys, FetchVerdict* v, hipStream_t st) {
    hipLaunchKernelGGL(k_fetch_verdict, dim3(1), dim3(1), 0, st, bad, keys, v);
    return hipGetLastError();
}

}  // namespace dml

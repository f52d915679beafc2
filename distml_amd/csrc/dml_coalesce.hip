// dml_coalesce.hip — the device gradient coalescer (C-ABI dml_coalescer_create / _destroy,
// dml_coalesce_device, dml_diag_coalesce_times).
//
// The reference worker fetches through a KeyList, a HashSet<Long> (KeyList.java:14-19,59-61),
// and accumulates its update per key in a HashMap before SparseMatrix.push writes one record
// per entry (SparseMatrix.java:46-60). A worker whose tensors are in HBM has occurrences: keys
// with repeats and one gradient row per occurrence. This call is that KeyList + HashMap pair on
// the device: the distinct keys ascending, for every occurrence the place of its key among
// them, and per key the sum of its rows in list order from +0.0: what a zero-initialised
// reference store holds after one handlePush of the occurrences (FloatMatrixStore.java:200-222).
//
//   k_co_pairs    (key ^ sign bit, occurrence index) pairs; hipcub's stable radix sort orders
//                 them, so the indices of one key stay in list order
//   k_co_heads    over the sorted keys, kCoBlockKeys per block: head flag key[i] != key[i-1],
//                 a block scan. <false> leaves the block's head count; k_co_offsets turns the
//                 counts into carried block offsets and the total, which the host reads;
//                 <true>, after the host's capacity check, writes keys_out[u], the segment
//                 start of u and inverse[index[i]] = u
//   k_co_sum      the ordered segmented gather-sum, output-stationary: a group of G lanes owns
//                 one 16-byte vector each of one output row's span (rows over 1 KiB are cut
//                 into 1-KiB spans), a wave carries 64 / G neighbouring items, so its stores
//                 are one contiguous run. A group walks its own segment: up to kCoBatch
//                 occurrence indices fetched one per lane and broadcast, kCoDepth rows' loads
//                 issued before the first add, adds strictly in occurrence order.
//   k_co_sum_narrow  rows under 16 bytes (arrays, 1-3 f32 / i32 columns, one f64): one lane per key
//
// The variant is chosen by the value type and the row width alone, so there is no knob.
#include <hipcub/hipcub.hpp>

#include "distml_ps.h"
#include "dml_fetch_line.h"
#include "dml_host.h"

using namespace dml;

namespace {

constexpr int kCoBlock = 256;
constexpr int kCoKeysPerThread = 4;
constexpr int kCoBlockKeys = kCoBlock * kCoKeysPerThread;
constexpr int kCoBatch = 16;  // indices a group fetches at a time (a group of G < 16 lanes: G)
constexpr int kCoDepth = 4;   // rows whose loads are issued before the first add
static_assert(kCoBlockKeys == DML_COALESCE_BLOCK_KEYS && kCoBatch == DML_COALESCE_BATCH &&
                  kCoDepth == DML_COALESCE_DEPTH && kCoBatch % kCoDepth == 0,
              "exported tile sizes");
constexpr uint64_t kSignBit = 1ull << 63;  // signed order as unsigned order
constexpr int64_t kCoSpanBytes = 1024;     // 64 lanes x 16 bytes
constexpr int64_t kCoMaxBlocks = (int64_t)1 << 22;

__device__ inline uint32_t ldg32_nt(const uint8_t* p) {
    return __builtin_nontemporal_load((const DML_GLOBAL uint32_t*)(p));
}

__global__ __launch_bounds__(kCoBlock) void k_co_pairs(const int64_t* __restrict__ keys, int64_t n,
                                                       uint64_t* __restrict__ kin, uint32_t* __restrict__ vin) {
    const int64_t i = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (i >= n) return;
    kin[i] = (uint64_t)keys[i] ^ kSignBit;
    vin[i] = (uint32_t)i;
}

// Inclusive scan of one value per thread over the block's 256 threads: returns this thread's
// inclusive sum and, in *before, the sum of the waves before its own. `wsum` is 4 LDS words.
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t* before, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t b = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCoBlock / 64; ++w) {
        if (w < wave) b += wsum[w];
        all += wsum[w];
    }
    *before = b;
    *total = all;
    return incl;
}

// WRITE false: blockoff[block] = the block's head count. WRITE true: blockoff holds the heads
// before the block (k_co_offsets), and the unique keys, segment starts and inverse are written.
template <bool WRITE>
__global__ __launch_bounds__(kCoBlock) void k_co_heads(const uint64_t* __restrict__ sk, const uint32_t* __restrict__ si,
                                                       int64_t n, uint32_t* __restrict__ blockoff,
                                                       int64_t* __restrict__ keys_out, uint32_t* __restrict__ seg,
                                                       int32_t* __restrict__ inverse) {
    __shared__ uint32_t wsum[kCoBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kCoBlockKeys + (int64_t)threadIdx.x * kCoKeysPerThread;
    uint64_t k[kCoKeysPerThread];
    uint64_t prev = (i0 > 0 && i0 - 1 < n) ? sk[i0 - 1] : 0;
    uint32_t flags = 0;
#pragma unroll
    for (int e = 0; e < kCoKeysPerThread; ++e) {
        const int64_t i = i0 + e;
        k[e] = i < n ? sk[i] : 0;
        if (i < n && (i == 0 || k[e] != prev)) flags |= 1u << e;
        prev = k[e];
    }
    const uint32_t cnt = (uint32_t)__popc(flags);
    uint32_t before, total;
    const uint32_t incl = block_scan(cnt, wsum, &before, &total);
    if (!WRITE) {
        if (threadIdx.x == 0) blockoff[blockIdx.x] = total;
        return;
    }
    uint32_t u = blockoff[blockIdx.x] + before + incl - cnt;  // the heads before this thread's first key
#pragma unroll
    for (int e = 0; e < kCoKeysPerThread; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) break;
        if (flags & (1u << e)) {
            keys_out[u] = (int64_t)(k[e] ^ kSignBit);
            seg[u] = (uint32_t)i;
            ++u;
        }
        if (inverse) inverse[si[i]] = (int32_t)(u - 1);  // key 0 is a head, so u >= 1 here
    }
}

// One block: blockoff[0..nb) from counts to the exclusive running sum, carried from one
// 256-count tile to the next; *count = the number of heads.
__global__ __launch_bounds__(kCoBlock) void k_co_offsets(uint32_t* __restrict__ blockoff, int64_t nb,
                                                         uint32_t* __restrict__ count) {
    __shared__ uint32_t wsum[kCoBlock / 64];
    uint32_t carry = 0;
    for (int64_t base = 0; base < nb; base += kCoBlock) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? blockoff[i] : 0;
        uint32_t before, total;
        const uint32_t incl = block_scan(v, wsum, &before, &total);
        if (i < nb) blockoff[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();  // wsum is rewritten by the next tile
    }
    if (threadIdx.x == 0) *count = carry;
}

// One add as the reference's JVM on x86-64 makes it: rounded once (the build has
// -ffp-contract=off), and the NaN an invalid operation creates (Inf - Inf: neither operand
// is one) is that platform's NEGATIVE quiet NaN, 0xFFC00000 / 0xFFF8000000000000, where
// gfx950 would create the positive one. An operand's NaN passes through, quieted, as on both.
__device__ inline float add_ref(float a, float x) {
    const float r = __fadd_rn(a, x);
    return (r != r && a == a && x == x) ? __uint_as_float(0xFFC00000u) : r;
}
__device__ inline double add_ref(double a, double x) {
    const double r = __dadd_rn(a, x);
    return (r != r && a == a && x == x) ? __longlong_as_double((long long)0xFFF8000000000000ull) : r;
}

// acc + x per element of one 16-byte vector; int32 wraps.
template <typename T> __device__ inline u32x4 add_vec(u32x4 a, u32x4 x);
template <> __device__ inline u32x4 add_vec<float>(u32x4 a, u32x4 x) {
    u32x4 r;
    r.x = __float_as_uint(add_ref(__uint_as_float(a.x), __uint_as_float(x.x)));
    r.y = __float_as_uint(add_ref(__uint_as_float(a.y), __uint_as_float(x.y)));
    r.z = __float_as_uint(add_ref(__uint_as_float(a.z), __uint_as_float(x.z)));
    r.w = __float_as_uint(add_ref(__uint_as_float(a.w), __uint_as_float(x.w)));
    return r;
}
template <> __device__ inline u32x4 add_vec<int32_t>(u32x4 a, u32x4 x) { return a + x; }
template <> __device__ inline u32x4 add_vec<double>(u32x4 a, u32x4 x) {
    const double lo = add_ref(Elem<double>::from_bits(a.x, a.y), Elem<double>::from_bits(x.x, x.y));
    const double hi = add_ref(Elem<double>::from_bits(a.z, a.w), Elem<double>::from_bits(x.z, x.w));
    const uint64_t l = (uint64_t)__double_as_longlong(lo), h = (uint64_t)__double_as_longlong(hi);
    u32x4 r;
    r.x = (uint32_t)l; r.y = (uint32_t)(l >> 32); r.z = (uint32_t)h; r.w = (uint32_t)(h >> 32);
    return r;
}

struct SumP {
    const uint8_t* values;  // T[n][cols], 4-byte aligned
    const uint32_t* idx;    // occurrence indices, sorted by key, list order inside a key
    const uint32_t* seg;    // seg[u]: the first sorted position of unique key u
    uint8_t* out;           // T[m][cols], 4-byte aligned
    int64_t n, m;
    int64_t rowbytes;       // >= 16
    int64_t nspan;          // 1-KiB spans of a row
    int32_t lgG;            // log2 of the lanes of a group
};

// The sum starts at +0.0 and a sum of IEEE adds that starts there is never -0.0 (x + y is
// -0.0 only when both are) nor a signalling NaN, so adding the +0.0 of a slot past the
// segment's end leaves every accumulator as it is: the adds of a batch are unconditional.
//
// A row's last vector, when the row is no multiple of 16 bytes, is loaded shifted back so
// that it ends at the row's last byte (the row is >= 16 bytes, so the load stays inside it);
// its leading elements repeat the previous lane's sums and only the trailing dwords are stored.
template <typename T>
__global__ __launch_bounds__(kCoBlock) void k_co_sum(const SumP a) {
    const int lane = threadIdx.x & 63;
    const int G = 1 << a.lgG, gl = lane & (G - 1), per = 64 >> a.lgG;
    const int B = G < kCoBatch ? G : kCoBatch;
    const int64_t nitem = a.m * a.nspan;
    const int64_t nwave = (nitem + per - 1) / per;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (int64_t w = (int64_t)blockIdx.x * (kCoBlock / 64) + (threadIdx.x >> 6); w < nwave;
         w += (int64_t)gridDim.x * (kCoBlock / 64)) {
        const int64_t item = w * per + (lane >> a.lgG);
        const bool live = item < nitem;
        int64_t u = 0, span = 0;
        if (live) {
            u = a.nspan == 1 ? item : item / a.nspan;
            span = item - u * a.nspan;
        }
        const int64_t vb = (span * 64 + gl) * 16;  // this lane's vector, as a byte of the row
        const bool act = live && vb < a.rowbytes;
        const bool tail = act && vb + 16 > a.rowbytes;
        // a lane past the row's end (G rounds up) loads the last vector too: one address, one request
        const int64_t off = vb + 16 > a.rowbytes ? a.rowbytes - 16 : vb;
        uint32_t s = 0, e = 0;
        if (live) {
            s = a.seg[u];
            e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        }
        u32x4 acc = zero;
        for (uint32_t base = s; base < e; base += (uint32_t)B) {
            const int cnt = e - base < (uint32_t)B ? (int)(e - base) : B;
            const uint32_t mine = gl < cnt ? a.idx[base + gl] : 0u;
            int k0 = 0;
            for (; k0 + kCoDepth <= cnt; k0 += kCoDepth) {  // whole steps: every load is unconditional
                u32x4 x[kCoDepth];
#pragma unroll
                for (int d = 0; d < kCoDepth; ++d) {
                    const uint32_t j = (uint32_t)__shfl((int)mine, (k0 + d) & (G - 1), G);
                    x[d] = ldg16_nt(a.values + (int64_t)j * a.rowbytes + off);
                }
#pragma unroll
                for (int d = 0; d < kCoDepth; ++d) acc = add_vec<T>(acc, x[d]);
            }
            if (k0 < cnt) {  // the batch's last 1 .. kCoDepth - 1 rows
                u32x4 x[kCoDepth - 1];
#pragma unroll
                for (int d = 0; d < kCoDepth - 1; ++d) {
                    const uint32_t j = (uint32_t)__shfl((int)mine, (k0 + d) & (G - 1), G);
                    x[d] = zero;
                    if (k0 + d < cnt) x[d] = ldg16_nt(a.values + (int64_t)j * a.rowbytes + off);
                }
#pragma unroll
                for (int d = 0; d < kCoDepth - 1; ++d) acc = add_vec<T>(acc, x[d]);
            }
        }
        if (!act) continue;
        uint8_t* o = a.out + u * a.rowbytes + vb;
        if (!tail) {
            stg16_nt(o, acc);
        } else {  // the trailing (rowbytes - vb) / 4 dwords of the shifted vector
            const int first = 4 - (int)((a.rowbytes - vb) >> 2);
            const uint32_t q[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
            for (int d = 1; d < 4; ++d)
                if (d >= first) stg32_nt(o + 4 * (d - first), q[d]);
        }
    }
}

template <int RDW>
__device__ inline u32x4 load_narrow(const uint8_t* p) {
    u32x4 x = {0u, 0u, 0u, 0u};
    if (RDW == 2) {
        const u32x2 t = __builtin_nontemporal_load((const DML_GLOBAL u32x2_u*)p);
        x.x = t.x; x.y = t.y;
    } else {
        x.x = ldg32_nt(p);
        if (RDW == 3) { x.y = ldg32_nt(p + 4); x.z = ldg32_nt(p + 8); }
    }
    return x;
}

// Rows of RDW = 1, 2 or 3 dwords: one lane per unique key, kCoDepth occurrences' indices
// and then their rows loaded before the adds.
template <typename T, int RDW>
__global__ __launch_bounds__(kCoBlock) void k_co_sum_narrow(const uint8_t* __restrict__ values,
                                                            const uint32_t* __restrict__ idx,
                                                            const uint32_t* __restrict__ seg, int64_t n, int64_t m,
                                                            uint8_t* __restrict__ out) {
    const int64_t u = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (u >= m) return;
    const uint32_t s = seg[u], e = u + 1 < m ? seg[u + 1] : (uint32_t)n;
    u32x4 acc = {0u, 0u, 0u, 0u};
    uint32_t k0 = s;
    for (; k0 + kCoDepth <= e; k0 += kCoDepth) {  // whole steps
        uint32_t j[kCoDepth];
        u32x4 x[kCoDepth];
#pragma unroll
        for (int d = 0; d < kCoDepth; ++d) j[d] = idx[k0 + d];
#pragma unroll
        for (int d = 0; d < kCoDepth; ++d) x[d] = load_narrow<RDW>(values + (int64_t)j[d] * (RDW * 4));
#pragma unroll
        for (int d = 0; d < kCoDepth; ++d) acc = add_vec<T>(acc, x[d]);
    }
    for (; k0 < e; ++k0)  // the last 1 .. kCoDepth - 1 occurrences
        acc = add_vec<T>(acc, load_narrow<RDW>(values + (int64_t)idx[k0] * (RDW * 4)));
    uint8_t* o = out + u * (RDW * 4);
    stg32_nt(o, acc.x);
    if (RDW >= 2) stg32_nt(o + 4, acc.y);
    if (RDW >= 3) stg32_nt(o + 8, acc.z);
}

template <typename T>
void launch_sum(const SumP& a, hipStream_t st) {
    if (a.rowbytes < 16) {
        const dim3 grid((unsigned)((a.m + kCoBlock - 1) / kCoBlock)), blk(kCoBlock);
        switch ((int)(a.rowbytes / 4)) {
            case 1: hipLaunchKernelGGL((k_co_sum_narrow<T, 1>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out); break;
            case 2: hipLaunchKernelGGL((k_co_sum_narrow<T, 2>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out); break;
            default: hipLaunchKernelGGL((k_co_sum_narrow<T, 3>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out); break;
        }
        return;
    }
    const int64_t per = 64 >> a.lgG, nwave = (a.m * a.nspan + per - 1) / per;
    const int64_t blocks = std::min<int64_t>((nwave + kCoBlock / 64 - 1) / (kCoBlock / 64), kCoMaxBlocks);
    hipLaunchKernelGGL((k_co_sum<T>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
}

bool overlap(const void* a, int64_t alen, const void* b, int64_t blen) {
    if (!a || !b || alen <= 0 || blen <= 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)blen && y < x + (uintptr_t)alen;
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

struct dml_coalescer {
    int device = 0;
    uint8_t* ws = nullptr;  // the workspace, grown on demand
    size_t ws_bytes = 0;
    uint32_t* count_dev = nullptr;  // k_co_offsets' total
    uint32_t* count_host = nullptr; // ... copied here (pinned); the one word the host waits for
    hipEvent_t done = nullptr;      // the last call's last kernel
    bool in_flight = false;
    hipEvent_t ev[6] = {};          // stage boundaries of the last call (dml_diag_coalesce_times)
    bool timed = false, timed_sum = false;
};

extern "C" int dml_coalescer_create(int32_t device, dml_coalescer** out) {
    if (!out) return set_error(DML_E_INVALID_ARG, "null out");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return set_error(DML_E_HIP, "no such HIP device");
    DeviceGuard g(device);
    dml_coalescer* c = new dml_coalescer;
    c->device = device;
    hipError_t e = hipMalloc((void**)&c->count_dev, 256);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->count_host, 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    if (e != hipSuccess) {
        const int rc = set_error(e == hipErrorOutOfMemory ? DML_E_NOMEM : DML_E_HIP,
                                 std::string("dml_coalescer_create: ") + hipGetErrorString(e));
        dml_coalescer_destroy(c);
        return rc;
    }
    *out = c;
    return DML_OK;
}

extern "C" void dml_coalescer_destroy(dml_coalescer* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    if (c->in_flight) (void)hipEventSynchronize(c->done);
    if (c->ws) (void)hipFree(c->ws);
    if (c->count_dev) (void)hipFree(c->count_dev);
    if (c->count_host) (void)hipHostFree(c->count_host);
    if (c->done) (void)hipEventDestroy(c->done);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
}

extern "C" int dml_coalesce_device(dml_coalescer* c, const dml_desc* desc, int32_t cols, const int64_t* dev_keys,
                                   int64_t n, const void* dev_values, int64_t* dev_keys_out, void* dev_values_out,
                                   int32_t* dev_inverse_out, int64_t cap_rows, int64_t* out_rows, void* stream) {
    // ---- argument checks: no HIP call, and `c` is not dereferenced, before they pass
    if (!c || !desc || !out_rows) return set_error(DML_E_INVALID_ARG, "null coalescer, desc or out_rows");
    const dml_desc d = *desc;
    if ((d.data_type != 0 && d.data_type != 1) || (d.key_type != 0 && d.key_type != 1) ||
        (d.value_type != DML_ELEMENT_TYPE_INT && d.value_type != DML_ELEMENT_TYPE_FLOAT &&
         d.value_type != DML_ELEMENT_TYPE_DOUBLE))
        return set_error(DML_E_BAD_DESC, "Unrecognized matrix type (DataStore.createStore)");
    const bool matrix = d.data_type == DML_DATA_TYPE_MATRIX;
    if (matrix && !d.dense_column)
        return set_error(DML_E_UNSUPPORTED, "sparse-column matrix rows are not supported (SURVEY defect 3)");
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative occurrence count");
    if (matrix && cols <= 0) return set_error(DML_E_INVALID_ARG, "cols must be > 0");
    if (n > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "lists of 2^31 occurrences and more");
    const int V = desc_value_bytes(d);
    const int64_t rowbytes = (int64_t)V * (matrix ? cols : 1);
    if (rowbytes / 4 > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "rows of 2^31 dwords and more");
    if ((((uintptr_t)dev_keys | (uintptr_t)dev_keys_out) & 7u) != 0)
        return set_error(DML_E_INVALID_ARG, "key array is not 8-byte aligned");
    if ((((uintptr_t)dev_values | (uintptr_t)dev_values_out | (uintptr_t)dev_inverse_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "values or inverse pointer is not 4-byte aligned");
    if (!dev_values && dev_values_out) return set_error(DML_E_INVALID_ARG, "values out without values");
    if (n > 0 && (!dev_keys || !dev_keys_out || (dev_values && !dev_values_out)))
        return set_error(DML_E_INVALID_ARG, "null keys, keys out or values out pointer");
    {
        // an output never extends past min(n, cap_rows) rows
        const int64_t mmax = cap_rows < 0 ? 0 : std::min(n, cap_rows);
        const void* in[2] = {dev_keys, dev_values};
        const int64_t inlen[2] = {n * 8, dev_values ? n * rowbytes : 0};
        const void* outp[3] = {dev_keys_out, dev_values_out, dev_inverse_out};
        const int64_t outlen[3] = {mmax * 8, dev_values_out ? mmax * rowbytes : 0, dev_inverse_out ? n * 4 : 0};
        for (int o = 0; o < 3; ++o) {
            for (int i = 0; i < 2; ++i)
                if (overlap(outp[o], outlen[o], in[i], inlen[i]))
                    return set_error(DML_E_INVALID_ARG, "coalesce output overlaps an input");
            for (int p = o + 1; p < 3; ++p)
                if (overlap(outp[o], outlen[o], outp[p], outlen[p]))
                    return set_error(DML_E_INVALID_ARG, "coalesce outputs overlap");
        }
    }
    if (n == 0) {
        *out_rows = 0;
        return DML_OK;
    }

    // ---- the device side
    DeviceGuard g(c->device);
    hipStream_t st = (hipStream_t)stream;
    if (c->in_flight) {  // one call in flight per context
        HIPCHK(hipEventSynchronize(c->done));
        c->in_flight = false;
    }
    c->timed = c->timed_sum = false;
    const int in = (int)n;
    const int64_t nb = (n + kCoBlockKeys - 1) / kCoBlockKeys;
    size_t tmp = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (const uint32_t*)nullptr, (uint32_t*)nullptr, in, 0, 64, st));
    // kin | kout | vin | vout | seg | blockoff | sort temp
    const size_t o_kin = 0, o_kout = o_kin + up256((size_t)n * 8), o_vin = o_kout + up256((size_t)n * 8),
                 o_vout = o_vin + up256((size_t)n * 4), o_seg = o_vout + up256((size_t)n * 4),
                 o_boff = o_seg + up256((size_t)n * 4), o_tmp = o_boff + up256((size_t)nb * 4),
                 need = o_tmp + up256(tmp);
    if (need > c->ws_bytes) {
        if (c->ws) (void)hipFree(c->ws);
        c->ws = nullptr;
        c->ws_bytes = 0;
        const size_t want = need + need / 4;
        if (hipMalloc((void**)&c->ws, want) != hipSuccess) {
            (void)hipGetLastError();
            return set_error(DML_E_NOMEM, "coalescer workspace");
        }
        c->ws_bytes = want;
    }
    uint64_t* kin = (uint64_t*)(c->ws + o_kin);
    uint64_t* kout = (uint64_t*)(c->ws + o_kout);
    uint32_t* vin = (uint32_t*)(c->ws + o_vin);
    uint32_t* vout = (uint32_t*)(c->ws + o_vout);
    uint32_t* seg = (uint32_t*)(c->ws + o_seg);
    uint32_t* boff = (uint32_t*)(c->ws + o_boff);
    const dim3 blk(kCoBlock);

    HIPCHK(hipEventRecord(c->ev[0], st));
    hipLaunchKernelGGL(k_co_pairs, dim3((unsigned)((n + kCoBlock - 1) / kCoBlock)), blk, 0, st, dev_keys, n, kin, vin);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(c->ws + o_tmp, tmp, (const uint64_t*)kin, kout, (const uint32_t*)vin,
                                              vout, in, 0, 64, st));
    HIPCHK(hipEventRecord(c->ev[1], st));
    hipLaunchKernelGGL((k_co_heads<false>), dim3((unsigned)nb), blk, 0, st, (const uint64_t*)kout,
                       (const uint32_t*)vout, n, boff, (int64_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_co_offsets, dim3(1), blk, 0, st, boff, nb, c->count_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->count_host, c->count_dev, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ev[2], st));
    // the one host wait: nothing is written to an output before the count is known to fit
    HIPCHK(hipEventSynchronize(c->ev[2]));
    const int64_t m = (int64_t)*c->count_host;
    *out_rows = m;
    if (m > cap_rows) return set_error(DML_E_CAPACITY, "more distinct keys than cap_rows");

    HIPCHK(hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL((k_co_heads<true>), dim3((unsigned)nb), blk, 0, st, (const uint64_t*)kout,
                       (const uint32_t*)vout, n, boff, dev_keys_out, seg, dev_inverse_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[4], st));
    if (dev_values) {
        SumP a;
        a.values = (const uint8_t*)dev_values;
        a.idx = vout;
        a.seg = seg;
        a.out = (uint8_t*)dev_values_out;
        a.n = n;
        a.m = m;
        a.rowbytes = rowbytes;
        a.nspan = (rowbytes + kCoSpanBytes - 1) / kCoSpanBytes;
        const int64_t nvec = std::min<int64_t>((rowbytes + 15) / 16, 64);
        a.lgG = 0;
        while (((int64_t)1 << a.lgG) < nvec) ++a.lgG;
        if (d.value_type == DML_ELEMENT_TYPE_FLOAT) launch_sum<float>(a, st);
        else if (d.value_type == DML_ELEMENT_TYPE_DOUBLE) launch_sum<double>(a, st);
        else launch_sum<int32_t>(a, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[5], st));
        c->timed_sum = true;
    }
    c->timed = true;
    HIPCHK(hipEventRecord(c->done, st));
    c->in_flight = true;
    if (!st) {
        HIPCHK(hipStreamSynchronize(st));
        c->in_flight = false;
    }
    return DML_OK;
}

extern "C" int dml_diag_coalesce_times(dml_coalescer* c, float* ms3) {
    if (!c || !ms3) return set_error(DML_E_INVALID_ARG, "null coalescer or ms3");
    if (!c->timed) return set_error(DML_E_INVALID_ARG, "no completed dml_coalesce_device on this context");
    DeviceGuard g(c->device);
    HIPCHK(hipEventSynchronize(c->done));
    c->in_flight = false;
    float order = 0, count = 0, write = 0, sum = 0;
    HIPCHK(hipEventElapsedTime(&order, c->ev[0], c->ev[1]));
    HIPCHK(hipEventElapsedTime(&count, c->ev[1], c->ev[2]));
    HIPCHK(hipEventElapsedTime(&write, c->ev[3], c->ev[4]));
    if (c->timed_sum) HIPCHK(hipEventElapsedTime(&sum, c->ev[4], c->ev[5]));
    ms3[0] = order;
    ms3[1] = count + write;
    ms3[2] = sum;
    return DML_OK;
}

// dml_coalesce.hip — the device gradient coalescer (C-ABI dml_coalescer_create / _destroy,
// dml_coalesce_device, dml_coalesce_pack_device, dml_coalesce_elems_device, dml_coalescer_set_long_min,
// dml_coalescer_set_key_range, dml_diag_coalesce_times / _route / _order).
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
//                 them, so the indices of one key stay in list order. With a key range
//                 declared (dml_coalescer_set_key_range) dml_coalesce_order.hip's passes leave
//                 the same two arrays instead, and these two run only if a key was outside it
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
// dml_coalesce_pack_device runs the same kernels with the sum kernels in their record form
// (REC): the sums go straight into push records, key in front, and no dense plane exists.
//
// dml::co_push_planes (dml_store_push_planes_device) runs the order, heads and count here and
// hands the sum to dml_push_planes.hip, whose kernels apply it to a store's shard (PushSink).
// dml::co_push_elems (dml_store_push_elems_device) does the same for element updates into an
// int32 store's checked adds (dml_push_elems.hip, ElemSink).
// dml_coalesce_elems_compact_device ends in dml_compact_rows.hip's count, scan and writing passes
// instead: compact update rows.
//
// A segment of the context's long_min occurrences and more is left out by both walks and
// summed by dml_coalesce_long.hip's kernels instead: the same adds in the same order.
#include <hipcub/hipcub.hpp>

#include "dml_coalesce_dev.h"

using namespace dml;

namespace {

constexpr int kCoKeysPerThread = 4;
constexpr int kCoBlockKeys = kCoBlock * kCoKeysPerThread;
constexpr int kCoBatch = 16;  // indices a group fetches at a time (a group of G < 16 lanes: G)
constexpr int kCoDepth = 4;   // rows whose loads are issued before the first add
static_assert(kCoBlockKeys == DML_COALESCE_BLOCK_KEYS && kCoBatch == DML_COALESCE_BATCH &&
                  kCoDepth == DML_COALESCE_DEPTH && kCoBatch % kCoDepth == 0,
              "exported tile sizes");
constexpr uint64_t kSignBit = 1ull << 63;  // signed order as unsigned order
constexpr int64_t kCoMaxBlocks = (int64_t)1 << 22;
constexpr int kRouteWord = 16;  // count_dev[16], [17]: long segments, their occurrences

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
// 256-count tile to the next; *count = the number of heads. It also clears the two route
// words behind the count (kRouteWord) for the call's long-segment list.
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
    if (threadIdx.x == 0) {
        *count = carry;
        count[kRouteWord] = 0;
        count[kRouteWord + 1] = 0;
    }
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
    uint32_t lmin;          // a segment of lmin occurrences and more is the long path's
    RecP rec;               // REC only: `out` is the records
};

// The sum starts at +0.0 and a sum of IEEE adds that starts there is never -0.0 (x + y is
// -0.0 only when both are) nor a signalling NaN, so adding the +0.0 of a slot past the
// segment's end leaves every accumulator as it is: the adds of a batch are unconditional.
//
// A row's last vector, when the row is no multiple of 16 bytes, is loaded shifted back so
// that it ends at the row's last byte (the row is >= 16 bytes, so the load stays inside it);
// its leading elements repeat the previous lane's sums and only the trailing dwords are stored.
//
// REC: the sums go to push record u's value field, and the lane that owns the row's first
// vector stores the key in front of it (RecP, dml_coalesce_dev.h). A record's value field is
// 4-byte aligned like a dense row, so the stores are the dense form's at another address.
template <typename T, bool REC>
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
        const bool lng = e - s >= a.lmin;  // the long path's: no walk and no store
        if (lng) e = s;
        int64_t key = 0;
        if constexpr (REC) {
            if (live && !lng && vb == 0) key = a.rec.ukeys[u];  // in flight over the walk
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
        if (!act || lng) continue;
        uint8_t* o;
        if constexpr (REC) {
            uint8_t* r = a.out + u * a.rec.stride;
            if (vb == 0) put_key(r, key, a.rec.kdw);
            o = r + 4 * a.rec.kdw + vb;
        } else {
            o = a.out + u * a.rowbytes + vb;
        }
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

// Rows of RDW = 1, 2 or 3 dwords: one lane per unique key, kCoDepth occurrences' indices
// and then their rows loaded before the adds.
// REC: the lane writes its whole record, key, row and pad, as ascending dwords.
template <typename T, int RDW, bool REC>
__global__ __launch_bounds__(kCoBlock) void k_co_sum_narrow(const uint8_t* __restrict__ values,
                                                            const uint32_t* __restrict__ idx,
                                                            const uint32_t* __restrict__ seg, int64_t n, int64_t m,
                                                            uint8_t* __restrict__ out, uint32_t lmin, const RecP rec) {
    const int64_t u = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (u >= m) return;
    const uint32_t s = seg[u], e = u + 1 < m ? seg[u + 1] : (uint32_t)n;
    if (e - s >= lmin) return;  // the long path's
    int64_t key = 0;
    if constexpr (REC) key = rec.ukeys[u];
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
    uint8_t* o;
    if constexpr (REC) {
        uint8_t* r = out + u * rec.stride;
        put_key(r, key, rec.kdw);
        o = r + 4 * rec.kdw;
    } else {
        o = out + u * (RDW * 4);
    }
    stg32_nt(o, acc.x);
    if (RDW >= 2) stg32_nt(o + 4, acc.y);
    if (RDW >= 3) stg32_nt(o + 8, acc.z);
    if constexpr (REC) {
        if (rec.pad) stg32_nt(o + RDW * 4, 0u);
    }
}

template <typename T, bool REC>
void launch_sum(const SumP& a, hipStream_t st) {
    if (a.rowbytes < 16) {
        const dim3 grid((unsigned)((a.m + kCoBlock - 1) / kCoBlock)), blk(kCoBlock);
        switch ((int)(a.rowbytes / 4)) {
            case 1: hipLaunchKernelGGL((k_co_sum_narrow<T, 1, REC>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out, a.lmin, a.rec); break;
            case 2: hipLaunchKernelGGL((k_co_sum_narrow<T, 2, REC>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out, a.lmin, a.rec); break;
            default: hipLaunchKernelGGL((k_co_sum_narrow<T, 3, REC>), grid, blk, 0, st, a.values, a.idx, a.seg, a.n, a.m, a.out, a.lmin, a.rec); break;
        }
        return;
    }
    const int64_t per = 64 >> a.lgG, nwave = (a.m * a.nspan + per - 1) / per;
    const int64_t blocks = std::min<int64_t>((nwave + kCoBlock / 64 - 1) / (kCoBlock / 64), kCoMaxBlocks);
    hipLaunchKernelGGL((k_co_sum<T, REC>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
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
    uint8_t* cr = nullptr;          // compact rows: the non-zero counts per (key, slice), grown on demand
    size_t cr_bytes = 0;
    hipEvent_t done = nullptr;      // the last call's last kernel
    hipEvent_t handoff = nullptr;   // plane push: the caller's stream, where the store's apply stream takes over
    bool in_flight = false;
    hipEvent_t ev[6] = {};          // stage boundaries of the last call (dml_diag_coalesce_times)
    bool timed = false, timed_sum = false;
    int64_t long_min = DML_COALESCE_LONG_MIN;  // dml_coalescer_set_long_min
    uint64_t kr_first = 0, kr_span = 0;  // dml_coalescer_set_key_range; span 0: none declared
    uint32_t epoch = 0;                  // what the bounded order stage's range check stores to count_dev[1]
    int32_t order[3] = {0, 0, 0};        // dml_diag_coalesce_order
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
    if (e == hipSuccess) e = hipMemset(c->count_dev, 0, 256);  // the flag word differs from every epoch
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->count_host, 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->handoff, hipEventDisableTiming);
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
    if (c->cr) (void)hipFree(c->cr);
    if (c->count_dev) (void)hipFree(c->count_dev);
    if (c->count_host) (void)hipHostFree(c->count_host);
    if (c->done) (void)hipEventDestroy(c->done);
    if (c->handoff) (void)hipEventDestroy(c->handoff);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
}

namespace {

// Where a call's results go: the dense form's planes, or the record form's stream.
struct CoOut {
    int64_t* keys_out;   // may be null in the record form: the keys then go to the workspace
    void* values_out;    // T[m][cols], or the push records
    int32_t* inverse;
    int64_t cap;         // rows, or bytes of the records
    int64_t rec_bytes;   // 0: dense; else the bytes of one push record
    int32_t kdw, pad;
    int64_t* out_len;    // record form: m x rec_bytes; dense form, when given: m x rowbytes
    // the compact form (dml_coalesce_elems_compact_device): ptr non-null, values_out null, cap in rows
    int32_t* ptr;
    int32_t* ecol;
    int32_t* eval;
    int64_t cap_entries;
    int64_t* out_entries;
};

// The third sum mode's input (dml_coalesce_elems_device): element updates instead of rows.
struct CoElems {
    const int32_t* cols;  // int32[n][per]
    const int32_t* vals;  // int32[n][per]
    int32_t ncols, per;
};

int co_run(dml_coalescer* c, const dml_desc& d, int64_t rowbytes, const int64_t* dev_keys, int64_t n,
           const void* dev_values, const CoElems* el, const CoOut& o, int64_t* out_rows, void* stream,
           const PushSink* sk = nullptr, const ElemSink* es = nullptr);

}  // namespace

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
    const CoOut o = {dev_keys_out, dev_values_out, dev_inverse_out, cap_rows, 0, 0, 0, nullptr};
    return co_run(c, d, rowbytes, dev_keys, n, dev_values, nullptr, o, out_rows, stream);
}

extern "C" int dml_coalesce_pack_device(dml_coalescer* c, const dml_desc* desc, int32_t cols, uint32_t flags,
                                        const int64_t* dev_keys, int64_t n, const void* dev_values,
                                        void* dev_records_out, int64_t cap_bytes, int64_t* dev_keys_out,
                                        int32_t* dev_inverse_out, int64_t* out_rows, int64_t* out_len, void* stream) {
    // ---- argument checks, the coalescer's and the pack's: no HIP call before they pass
    if (!c || !desc || !out_rows || !out_len)
        return set_error(DML_E_INVALID_ARG, "null coalescer, desc, out_rows or out_len");
    int64_t R = 0;
    if (int rc = dml_record_bytes(desc, cols, flags, &R, nullptr)) return rc;  // desc, flags, cols, record length
    const dml_desc d = *desc;
    const bool matrix = d.data_type == DML_DATA_TYPE_MATRIX;
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative occurrence count");
    if (n > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "lists of 2^31 occurrences and more");
    const int K = desc_key_bytes(d);
    const int64_t rowbytes = (int64_t)desc_value_bytes(d) * (matrix ? cols : 1);
    if (R / 4 > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "records of 2^31 dwords and more");
    if (n > 0 && R > INT64_MAX / n) return set_error(DML_E_INVALID_ARG, "occurrence count overflows the byte length");
    if ((((uintptr_t)dev_keys | (uintptr_t)dev_keys_out) & 7u) != 0)
        return set_error(DML_E_INVALID_ARG, "key array is not 8-byte aligned");
    if ((((uintptr_t)dev_values | (uintptr_t)dev_records_out | (uintptr_t)dev_inverse_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "values, records or inverse pointer is not 4-byte aligned");
    if (n > 0 && (!dev_keys || !dev_values || !dev_records_out))
        return set_error(DML_E_INVALID_ARG, "null keys, values or records pointer");
    {
        // the records never extend past min(n x R, cap_bytes) bytes, the keys past as many rows
        const int64_t rbytes = cap_bytes < 0 ? 0 : std::min(n * R, cap_bytes);
        const void* in[2] = {dev_keys, dev_values};
        const int64_t inlen[2] = {n * 8, n * rowbytes};
        const void* outp[3] = {dev_keys_out, dev_records_out, dev_inverse_out};
        const int64_t outlen[3] = {rbytes / R * 8, rbytes, dev_inverse_out ? n * 4 : 0};
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
        *out_len = 0;
        return DML_OK;
    }
    const CoOut o = {dev_keys_out, dev_records_out, dev_inverse_out, cap_bytes, R, K / 4,
                     R != K + rowbytes ? 1 : 0, out_len};
    return co_run(c, d, rowbytes, dev_keys, n, dev_values, nullptr, o, out_rows, stream);
}

extern "C" int dml_coalesce_elems_device(dml_coalescer* c, const dml_desc* desc, int32_t cols, uint32_t flags,
                                         const int64_t* dev_keys, int64_t n, int32_t per_occ, const int32_t* dev_cols,
                                         const int32_t* dev_vals, int32_t form, void* dev_out, int64_t cap_bytes,
                                         int64_t* dev_keys_out, int32_t* dev_inverse_out, int64_t* out_rows,
                                         int64_t* out_len, void* stream) {
    // ---- argument checks, the pack call's and the elements': no HIP call before they pass
    if (!c || !desc || !out_rows || !out_len)
        return set_error(DML_E_INVALID_ARG, "null coalescer, desc, out_rows or out_len");
    int64_t R = 0;
    if (int rc = dml_record_bytes(desc, cols, flags, &R, nullptr)) return rc;  // desc, flags, cols, record length
    const dml_desc d = *desc;
    if (d.data_type != DML_DATA_TYPE_MATRIX)
        return set_error(DML_E_UNSUPPORTED, "an array's element update is dml_coalesce_device with cols = 1");
    if (d.value_type != DML_ELEMENT_TYPE_INT || d.ada_grad)
        return set_error(DML_E_UNSUPPORTED, "element updates are int32 only: float sums depend on their order");
    if (form != DML_ELEMS_ROWS && form != DML_ELEMS_RECORDS) return set_error(DML_E_INVALID_ARG, "unknown output form");
    if (per_occ < 1 || per_occ > DML_COALESCE_ELEMS_MAX_PER_OCC)
        return set_error(DML_E_INVALID_ARG, "per_occ outside 1 .. DML_COALESCE_ELEMS_MAX_PER_OCC");
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative occurrence count");
    if (n > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "lists of 2^31 occurrences and more");
    const bool rec = form == DML_ELEMS_RECORDS;
    const int K = desc_key_bytes(d);
    const int64_t rowbytes = 4 * (int64_t)cols;
    const int64_t ob = rec ? R : rowbytes;  // bytes of one output row or record
    if (ob / 4 > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "rows or records of 2^31 dwords and more");
    if (n > 0 && ob > INT64_MAX / n) return set_error(DML_E_INVALID_ARG, "occurrence count overflows the byte length");
    if ((((uintptr_t)dev_keys | (uintptr_t)dev_keys_out) & 7u) != 0)
        return set_error(DML_E_INVALID_ARG, "key array is not 8-byte aligned");
    if ((((uintptr_t)dev_cols | (uintptr_t)dev_vals | (uintptr_t)dev_out | (uintptr_t)dev_inverse_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "columns, values, output or inverse pointer is not 4-byte aligned");
    if (n > 0 && (!dev_keys || !dev_cols || !dev_vals || !dev_out))
        return set_error(DML_E_INVALID_ARG, "null keys, columns, values or output pointer");
    if (n > 0 && !rec && !dev_keys_out) return set_error(DML_E_INVALID_ARG, "the row form needs dev_keys_out");
    {
        // the output never extends past min(n x ob, cap_bytes) bytes, the keys past as many rows
        const int64_t obytes = cap_bytes < 0 ? 0 : std::min(n * ob, cap_bytes);
        const void* in[3] = {dev_keys, dev_cols, dev_vals};
        const int64_t inlen[3] = {n * 8, n * per_occ * 4, n * per_occ * 4};
        const void* outp[3] = {dev_keys_out, dev_out, dev_inverse_out};
        const int64_t outlen[3] = {obytes / ob * 8, obytes, dev_inverse_out ? n * 4 : 0};
        for (int o = 0; o < 3; ++o) {
            for (int i = 0; i < 3; ++i)
                if (overlap(outp[o], outlen[o], in[i], inlen[i]))
                    return set_error(DML_E_INVALID_ARG, "coalesce output overlaps an input");
            for (int p = o + 1; p < 3; ++p)
                if (overlap(outp[o], outlen[o], outp[p], outlen[p]))
                    return set_error(DML_E_INVALID_ARG, "coalesce outputs overlap");
        }
    }
    if (n == 0) {
        *out_rows = 0;
        *out_len = 0;
        return DML_OK;
    }
    const CoElems el = {dev_cols, dev_vals, cols, per_occ};
    // the dense form's capacity in rows: m > cap_bytes / rowbytes exactly when m x rowbytes > cap_bytes
    const CoOut o = rec ? CoOut{dev_keys_out, dev_out, dev_inverse_out, cap_bytes, R, K / 4, 0, out_len}
                        : CoOut{dev_keys_out, dev_out, dev_inverse_out, cap_bytes < 0 ? -1 : cap_bytes / rowbytes, 0, 0, 0, out_len};
    return co_run(c, d, rowbytes, dev_keys, n, nullptr, &el, o, out_rows, stream);
}

extern "C" int dml_coalesce_elems_compact_device(dml_coalescer* c, const dml_desc* desc, int32_t cols,
                                                 const int64_t* dev_keys, int64_t n, int32_t per_occ,
                                                 const int32_t* dev_cols, const int32_t* dev_vals,
                                                 int64_t* dev_keys_out, int32_t* dev_ptr_out, int32_t* dev_ecol_out,
                                                 int32_t* dev_eval_out, int64_t cap_rows, int64_t cap_entries,
                                                 int32_t* dev_inverse_out, int64_t* out_rows, int64_t* out_entries,
                                                 void* stream) {
    // ---- argument checks, the element call's: no HIP call before they pass
    if (!c || !desc || !out_rows) return set_error(DML_E_INVALID_ARG, "null coalescer, desc or out_rows");
    if (int rc = dml_record_bytes(desc, cols, 0, nullptr, nullptr)) return rc;  // desc, cols
    const dml_desc d = *desc;
    if (d.data_type != DML_DATA_TYPE_MATRIX)
        return set_error(DML_E_UNSUPPORTED, "compact rows are matrix rows: an array's update is one value per key");
    if (d.value_type != DML_ELEMENT_TYPE_INT || d.ada_grad)
        return set_error(DML_E_UNSUPPORTED, "element updates are int32 only: float sums depend on their order");
    if (per_occ < 1 || per_occ > DML_COALESCE_ELEMS_MAX_PER_OCC)
        return set_error(DML_E_INVALID_ARG, "per_occ outside 1 .. DML_COALESCE_ELEMS_MAX_PER_OCC");
    if (n < 0) return set_error(DML_E_INVALID_ARG, "negative occurrence count");
    if (n * per_occ > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "lists of 2^31 elements and more: ptr is int32");
    if ((((uintptr_t)dev_keys | (uintptr_t)dev_keys_out) & 7u) != 0)
        return set_error(DML_E_INVALID_ARG, "key array is not 8-byte aligned");
    if ((((uintptr_t)dev_cols | (uintptr_t)dev_vals | (uintptr_t)dev_ptr_out | (uintptr_t)dev_ecol_out |
          (uintptr_t)dev_eval_out | (uintptr_t)dev_inverse_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "columns, values, ptr, entries or inverse pointer is not 4-byte aligned");
    if (n > 0 && (!dev_keys || !dev_cols || !dev_vals || !dev_keys_out || !dev_ptr_out || !dev_ecol_out || !dev_eval_out))
        return set_error(DML_E_INVALID_ARG, "null keys, columns, values or output pointer");
    {
        // no output extends past min(n, cap_rows) rows (+ 1 for ptr) or min(n x per_occ, cap_entries) entries
        const int64_t mmax = cap_rows < 0 ? 0 : std::min(n, cap_rows);
        const int64_t emax = cap_entries < 0 ? 0 : std::min(n * per_occ, cap_entries);
        const void* in[3] = {dev_keys, dev_cols, dev_vals};
        const int64_t inlen[3] = {n * 8, n * per_occ * 4, n * per_occ * 4};
        const void* outp[5] = {dev_keys_out, dev_ptr_out, dev_ecol_out, dev_eval_out, dev_inverse_out};
        const int64_t outlen[5] = {mmax * 8, n > 0 ? (mmax + 1) * 4 : 0, emax * 4, emax * 4, dev_inverse_out ? n * 4 : 0};
        for (int o = 0; o < 5; ++o) {
            for (int i = 0; i < 3; ++i)
                if (overlap(outp[o], outlen[o], in[i], inlen[i]))
                    return set_error(DML_E_INVALID_ARG, "coalesce output overlaps an input");
            for (int p = o + 1; p < 5; ++p)
                if (overlap(outp[o], outlen[o], outp[p], outlen[p]))
                    return set_error(DML_E_INVALID_ARG, "coalesce outputs overlap");
        }
    }
    if (n == 0) {  // an empty list has no ptr either: nothing is written
        *out_rows = 0;
        if (out_entries) *out_entries = 0;
        return DML_OK;
    }
    const CoElems el = {dev_cols, dev_vals, cols, per_occ};
    const CoOut o = {dev_keys_out, nullptr, dev_inverse_out, cap_rows, 0, 0, 0, nullptr,
                     dev_ptr_out, dev_ecol_out, dev_eval_out, cap_entries, out_entries};
    return co_run(c, d, 4 * (int64_t)cols, dev_keys, n, nullptr, &el, o, out_rows, stream);
}

namespace {

// The device side of the three calls, after their argument checks. The sum is dense or
// record (`o`) over rows (`dev_values`) or over element updates (`el`; then `rowbytes` is the
// output row's). `sk` (co_push_planes) or `es` (co_push_elems): the sink is a store; `o` then names no output, the
// distinct keys stay in the workspace, and the sum kernels, the store's verdict and `done` go
// on its apply stream behind an event of `stream` (a null `stream`: every stage runs there,
// and the caller synchronises).
int co_run(dml_coalescer* c, const dml_desc& d, int64_t rowbytes, const int64_t* dev_keys, int64_t n,
           const void* dev_values, const CoElems* el, const CoOut& o, int64_t* out_rows, void* stream,
           const PushSink* sk, const ElemSink* es) {
    DeviceGuard g(c->device);
    hipStream_t st = (hipStream_t)stream;
    const hipStream_t apply = sk ? sk->apply : es ? es->apply : nullptr;  // a store sink's stream
    if ((sk || es) && !st) st = apply;
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
    // a segment of lmin occurrences and more takes the long path; 2^31: none does (n < 2^31)
    const uint32_t lmin = (uint32_t)std::min<int64_t>(c->long_min, (int64_t)1 << 31);
    const int64_t nlong = dev_values || el ? n / lmin : 0;  // the most long segments n occurrences hold
    const bool rec = o.rec_bytes != 0;
    const size_t ukeys = (rec || sk || es) && !o.keys_out ? (size_t)n * 8 : 0;  // the record form and the sink read the keys back
    // kin | kout | vin | vout | seg | blockoff | long list | unique keys | sort temp
    const size_t o_kin = 0, o_kout = o_kin + up256((size_t)n * 8), o_vin = o_kout + up256((size_t)n * 8),
                 o_vout = o_vin + up256((size_t)n * 4), o_seg = o_vout + up256((size_t)n * 4),
                 o_boff = o_seg + up256((size_t)n * 4), o_list = o_boff + up256((size_t)nb * 4), o_uk = o_list + up256((size_t)nlong * 4), o_tmp = o_uk + up256(ukeys);
    // A declared key range: the bounded order stage (dml_coalesce_order.hip). Its second word
    // buffer and its counts lie where the library sort's temporaries do; its first is kin.
    const bool bounded = c->kr_span != 0 && co_order_passes(c->kr_span) <= DML_COALESCE_ORDER_MAX_PASSES;
    const size_t o_cnt = o_tmp + up256((size_t)n * 8);
    const size_t need = std::max(o_tmp + up256(tmp), bounded ? o_cnt + up256(co_order_count_bytes()) : 0);
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

    c->order[0] = c->order[1] = c->order[2] = 0;
    if (bounded && ++c->epoch == 0) c->epoch = 1;
    for (int attempt = 0;; ++attempt) {
        const bool own = bounded && attempt == 0;
        HIPCHK(hipEventRecord(c->ev[0], st));
        if (own) {
            const OrderP op = {dev_keys, n, c->kr_first, c->kr_span, kin, (uint64_t*)(c->ws + o_tmp),
                               (uint32_t*)(c->ws + o_cnt), kout, vout, c->count_dev + 1, c->epoch};
            co_launch_order(op, st);
            HIPCHK(hipGetLastError());
        } else {
            hipLaunchKernelGGL(k_co_pairs, dim3((unsigned)((n + kCoBlock - 1) / kCoBlock)), blk, 0, st, dev_keys, n, kin, vin);
            HIPCHK(hipGetLastError());
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(c->ws + o_tmp, tmp, (const uint64_t*)kin, kout, (const uint32_t*)vin,
                                                      vout, in, 0, 64, st));
        }
        HIPCHK(hipEventRecord(c->ev[1], st));
        hipLaunchKernelGGL((k_co_heads<false>), dim3((unsigned)nb), blk, 0, st, (const uint64_t*)kout,
                           (const uint32_t*)vout, n, boff, (int64_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr);
        hipLaunchKernelGGL(k_co_offsets, dim3(1), blk, 0, st, boff, nb, c->count_dev);
        HIPCHK(hipGetLastError());
        // the count and, beside it, the range check's flag word
        HIPCHK(hipMemcpyAsync(c->count_host, c->count_dev, own ? 8 : 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c->ev[2], st));
        // the one host wait: nothing is written to an output before the count is known to fit
        HIPCHK(hipEventSynchronize(c->ev[2]));
        if (!own) break;
        if (c->count_host[1] != c->epoch) {  // every key was inside the declared range
            c->order[0] = 1;
            c->order[1] = co_order_passes(c->kr_span);
            break;
        }
        c->order[2] = 1;  // a key outside it: the library sort orders the list, and a second wait
    }
    const int64_t m = (int64_t)*c->count_host;
    *out_rows = m;
    if (rec) {
        *o.out_len = m * o.rec_bytes;
        if (m * o.rec_bytes > o.cap) return set_error(DML_E_CAPACITY, "coalesced push records exceed cap_bytes");
    } else {
        if (o.out_len) *o.out_len = m * rowbytes;
        if (m > o.cap) return set_error(DML_E_CAPACITY, "more distinct keys than cap_rows");
    }
    int64_t nitem = 0;
    if (o.ptr) {
        // nnz is known only on the device, and this call waits once. So cap_entries is held to the
        // bound the host does know, nnz <= min(n x per_occ, m x cols): a capacity under it is refused
        // here, before any write, whatever nnz turns out to be, and one at or above it cannot be short.
        const int64_t bound = std::min(n * el->per, m > INT64_MAX / el->ncols ? INT64_MAX : m * el->ncols);
        if (o.cap_entries < bound)
            return set_error(DML_E_CAPACITY, "cap_entries is under min(n x per_occ, m x cols), the bound on the entries");
        nitem = m * co_elems_slices(el->ncols);
        if (nitem > 0x7FFFFFFFll) return set_error(DML_E_UNSUPPORTED, "2^31 (key, slice) items and more");
        const size_t need_cr = ((size_t)nitem + 1) * 4;
        if (need_cr > c->cr_bytes) {  // the per-item counts; grown here because m was not known before
            if (c->cr) (void)hipFree(c->cr);
            c->cr = nullptr;
            c->cr_bytes = 0;
            if (hipMalloc((void**)&c->cr, need_cr + need_cr / 4) != hipSuccess) {
                (void)hipGetLastError();
                return set_error(DML_E_NOMEM, "coalescer compact-row counts");
            }
            c->cr_bytes = need_cr + need_cr / 4;
        }
    }
    int64_t* keys_out = o.keys_out ? o.keys_out : (int64_t*)(c->ws + o_uk);

    HIPCHK(hipEventRecord(c->ev[3], st));
    hipLaunchKernelGGL((k_co_heads<true>), dim3((unsigned)nb), blk, 0, st, (const uint64_t*)kout,
                       (const uint32_t*)vout, n, boff, keys_out, seg, o.inverse);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[4], st));
    if (el && es) {
        PushElemsP a;
        a.e.cols = el->cols;
        a.e.vals = el->vals;
        a.e.idx = vout;
        a.e.seg = seg;
        a.e.out = nullptr;
        a.e.n = n;
        a.e.m = m;
        a.e.rowbytes = rowbytes;
        a.e.nslice = co_elems_slices(el->ncols);
        a.e.ncols = el->ncols;
        a.e.per = el->per;
        a.e.lmin = lmin;
        a.e.list = (uint32_t*)(c->ws + o_list);
        a.e.route = c->count_dev + kRouteWord;
        a.e.rec = RecP{};
        a.ukeys = keys_out;
        a.sink = *es;
        if (st != apply) {  // the inputs and the order are complete on `st`: no host wait
            HIPCHK(hipEventRecord(c->handoff, st));
            HIPCHK(hipStreamWaitEvent(apply, c->handoff, 0));
        }
        HIPCHK(launch_push_elems(a, nlong > 0, apply));
        HIPCHK(hipEventRecord(c->ev[5], apply));
        c->timed_sum = true;
    } else if (el && o.ptr) {
        CompactP a;
        a.e.cols = el->cols;
        a.e.vals = el->vals;
        a.e.idx = vout;
        a.e.seg = seg;
        a.e.out = nullptr;
        a.e.n = n;
        a.e.m = m;
        a.e.rowbytes = rowbytes;
        a.e.nslice = co_elems_slices(el->ncols);
        a.e.ncols = el->ncols;
        a.e.per = el->per;
        a.e.lmin = lmin;
        a.e.list = (uint32_t*)(c->ws + o_list);
        a.e.route = c->count_dev + kRouteWord;
        a.e.rec = RecP{};
        a.ptr = o.ptr;
        a.ecol = o.ecol;
        a.eval = o.eval;
        a.cnt = (uint32_t*)c->cr;
        co_launch_compact(a, nlong > 0, st);
        HIPCHK(hipGetLastError());
        if (o.out_entries)  // ptr[m], behind the writing pass; read after the wait on `done` below
            HIPCHK(hipMemcpyAsync(c->count_host + 2, o.ptr + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(c->ev[5], st));
        c->timed_sum = true;
    } else if (el) {
        ElemsP a;
        a.cols = el->cols;
        a.vals = el->vals;
        a.idx = vout;
        a.seg = seg;
        a.out = (uint8_t*)o.values_out;
        a.n = n;
        a.m = m;
        a.rowbytes = rowbytes;
        a.nslice = co_elems_slices(el->ncols);
        a.ncols = el->ncols;
        a.per = el->per;
        a.lmin = lmin;
        a.list = (uint32_t*)(c->ws + o_list);
        a.route = c->count_dev + kRouteWord;
        a.rec = RecP{keys_out, o.rec_bytes, o.kdw, o.pad};
        co_launch_elems(a, rec, nlong > 0, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[5], st));
        c->timed_sum = true;
    } else if (sk) {
        PushP a;
        a.values = (const uint8_t*)dev_values;
        a.idx = vout;
        a.seg = seg;
        a.ukeys = keys_out;
        a.n = n;
        a.m = m;
        a.rowbytes = rowbytes;
        a.nspan = (rowbytes + kCoSpanBytes - 1) / kCoSpanBytes;
        const int64_t nvec = std::min<int64_t>((rowbytes + 15) / 16, 64);
        a.lgG = 0;
        while (((int64_t)1 << a.lgG) < nvec) ++a.lgG;
        a.lmin = lmin;
        a.list = (uint32_t*)(c->ws + o_list);
        a.route = c->count_dev + kRouteWord;
        a.sink = *sk;
        a.cand = sk->cand;
        if (st != sk->apply) {  // the inputs and the order are complete on `st`: no host wait
            HIPCHK(hipEventRecord(c->handoff, st));
            HIPCHK(hipStreamWaitEvent(sk->apply, c->handoff, 0));
        }
        HIPCHK(launch_push_planes(a, d.value_type, nlong > 0, sk->apply));
        HIPCHK(launch_fetch_verdict(sk->bad, keys_out, const_cast<FetchVerdict*>(sk->verdict), sk->apply));
        HIPCHK(hipEventRecord(c->ev[5], sk->apply));
        c->timed_sum = true;
    } else if (dev_values) {
        SumP a;
        a.values = (const uint8_t*)dev_values;
        a.idx = vout;
        a.seg = seg;
        a.out = (uint8_t*)o.values_out;
        a.n = n;
        a.m = m;
        a.rowbytes = rowbytes;
        a.nspan = (rowbytes + kCoSpanBytes - 1) / kCoSpanBytes;
        const int64_t nvec = std::min<int64_t>((rowbytes + 15) / 16, 64);
        a.lgG = 0;
        while (((int64_t)1 << a.lgG) < nvec) ++a.lgG;
        a.lmin = lmin;
        a.rec = RecP{keys_out, o.rec_bytes, o.kdw, o.pad};
        if (nlong > 0) {  // the list, then the long sums; the walks below skip what they take
            LongP l;
            l.values = a.values;
            l.idx = vout;
            l.seg = seg;
            l.out = a.out;
            l.n = n;
            l.m = m;
            l.rowbytes = rowbytes;
            l.lmin = lmin;
            l.list = (uint32_t*)(c->ws + o_list);
            l.route = c->count_dev + kRouteWord;
            l.rec = a.rec;
            co_launch_long(l, d.value_type, rec, st);
            HIPCHK(hipGetLastError());
        }
        const int vt = d.value_type;
        if (rec) {
            if (vt == DML_ELEMENT_TYPE_FLOAT) launch_sum<float, true>(a, st);
            else if (vt == DML_ELEMENT_TYPE_DOUBLE) launch_sum<double, true>(a, st);
            else launch_sum<int32_t, true>(a, st);
        } else {
            if (vt == DML_ELEMENT_TYPE_FLOAT) launch_sum<float, false>(a, st);
            else if (vt == DML_ELEMENT_TYPE_DOUBLE) launch_sum<double, false>(a, st);
            else launch_sum<int32_t, false>(a, st);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[5], st));
        c->timed_sum = true;
    }
    c->timed = true;
    HIPCHK(hipEventRecord(c->done, apply ? apply : st));
    c->in_flight = true;
    if (!st) {
        HIPCHK(hipStreamSynchronize(st));
        c->in_flight = false;
    }
    if (o.out_entries) {  // the compact form's second wait: for the whole call, whose last copy this is
        HIPCHK(hipEventSynchronize(c->done));
        c->in_flight = false;
        *o.out_entries = (int64_t)c->count_host[2];
    }
    return DML_OK;
}

}  // namespace

int dml::co_device(const dml_coalescer* c) { return c->device; }

int dml::co_push_planes(dml_coalescer* c, int32_t value_type, int64_t rowbytes, const int64_t* dev_keys, int64_t n,
                        const void* dev_values, const PushSink& sk, void* stream) {
    dml_desc d{};
    d.value_type = value_type;
    const CoOut o = {nullptr, nullptr, nullptr, n, 0, 0, 0, nullptr};  // no output: m <= n always fits
    int64_t m = 0;
    return co_run(c, d, rowbytes, dev_keys, n, dev_values, nullptr, o, &m, stream, &sk);
}

int dml::co_push_elems(dml_coalescer* c, const int64_t* dev_keys, int64_t n, int32_t per_occ, const int32_t* dev_cols,
                       const int32_t* dev_vals, const ElemSink& sk, void* stream) {
    dml_desc d{};
    d.value_type = DML_ELEMENT_TYPE_INT;
    const CoOut o = {nullptr, nullptr, nullptr, n, 0, 0, 0, nullptr};  // no output: m <= n always fits
    const CoElems el = {dev_cols, dev_vals, sk.cols, per_occ};
    int64_t m = 0;
    return co_run(c, d, 4 * (int64_t)sk.cols, dev_keys, n, nullptr, &el, o, &m, stream, nullptr, &sk);
}

extern "C" int dml_diag_coalesce_times(dml_coalescer* c, float* ms3) {
    if (!c || !ms3) return set_error(DML_E_INVALID_ARG, "null coalescer or ms3");
    if (!c->timed) return set_error(DML_E_INVALID_ARG, "no completed dml_coalesce_device or dml_coalesce_pack_device on this context");
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

extern "C" int dml_coalescer_set_long_min(dml_coalescer* c, int64_t v) {
    if (!c) return set_error(DML_E_INVALID_ARG, "null coalescer");
    if (v < 0) return set_error(DML_E_INVALID_ARG, "negative long_min");
    c->long_min = v == 0 ? DML_COALESCE_LONG_MIN : v;
    return DML_OK;
}

extern "C" int dml_coalescer_set_key_range(dml_coalescer* c, int64_t first, int64_t last) {
    if (!c) return set_error(DML_E_INVALID_ARG, "null coalescer");
    if (first > last) return set_error(DML_E_INVALID_ARG, "key range with first > last");
    const uint64_t span = (uint64_t)last - (uint64_t)first;
    if (span > (1ull << 32)) return set_error(DML_E_UNSUPPORTED, "key ranges of more than 2^32 keys");
    c->kr_first = span ? (uint64_t)first : 0;  // first == last: no declaration
    c->kr_span = span;
    return DML_OK;
}

extern "C" int dml_diag_coalesce_order(dml_coalescer* c, int32_t* out3) {
    if (!c || !out3) return set_error(DML_E_INVALID_ARG, "null coalescer or out");
    if (!c->timed) return set_error(DML_E_INVALID_ARG, "no completed dml_coalesce_device or dml_coalesce_pack_device on this context");
    DeviceGuard g(c->device);
    HIPCHK(hipEventSynchronize(c->done));
    c->in_flight = false;
    for (int i = 0; i < 3; ++i) out3[i] = c->order[i];
    return DML_OK;
}

extern "C" int dml_diag_coalesce_route(dml_coalescer* c, int64_t* out2) {
    if (!c || !out2) return set_error(DML_E_INVALID_ARG, "null coalescer or out");
    if (!c->timed) return set_error(DML_E_INVALID_ARG, "no completed dml_coalesce_device or dml_coalesce_pack_device on this context");
    DeviceGuard g(c->device);
    HIPCHK(hipEventSynchronize(c->done));
    c->in_flight = false;
    uint32_t w[2] = {0u, 0u};
    if (c->timed_sum) HIPCHK(hipMemcpy(w, c->count_dev + kRouteWord, 8, hipMemcpyDeviceToHost));
    out2[0] = w[0];
    out2[1] = w[1];
    return DML_OK;
}

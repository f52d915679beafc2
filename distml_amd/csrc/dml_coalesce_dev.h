// dml_coalesce_dev.h — what the coalescer's kernel files share (dml_coalesce.hip: order,
// heads and the walk k_co_sum; dml_coalesce_long.hip: the long-segment list and its sum
// kernels; dml_coalesce_elems.hip: the element-update sum; dml_coalesce_order.hip: the order
// stage for keys in a declared range): the one add
// of the contract, the narrow row load, the record form's parameters, the long path's and
// the element sum's launches, and the store-sink form of the sum (dml_push_planes.hip,
// §4.17). Device and host; not part of the public ABI.
#pragma once
#include "distml_ps.h"
#include "dml_fetch_line.h"
#include "dml_host.h"

namespace dml {

constexpr int kCoBlock = 256;
constexpr int64_t kCoSpanBytes = 1024;  // 64 lanes x 16 bytes

__device__ inline uint32_t ldg32_nt(const uint8_t* p) {
    return __builtin_nontemporal_load((const DML_GLOBAL uint32_t*)(p));
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
__device__ inline int32_t add_ref(int32_t a, int32_t x) { return (int32_t)((uint32_t)a + (uint32_t)x); }

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

// The record form of the sum kernels (dml_coalesce_pack_device; their REC instantiations):
// `out` is then the push records' first byte and key u's sums go to record u's value field,
// out + u x stride + 4 x kdw, behind the key that the lane (thread) storing the row's first
// element writes just before it, and in front of a float array record's zero pad, so one
// record, and with it one wave's records, leaves as one run of ascending stores. The dense
// instantiations read none of this.
struct RecP {
    const int64_t* ukeys;  // the distinct keys, ascending (k_co_heads<true>'s keys_out)
    int64_t stride;        // bytes of one push record
    int32_t kdw;           // dwords of its key field: 1 or 2
    int32_t pad;           // 1: FloatArrayStore's [f32][4 zero bytes] slot
};

// The key field of the record at `r`: the low kdw dwords of the key, little-endian (a 4-byte
// key is the writer's (int) cast).
__device__ inline void put_key(uint8_t* r, int64_t key, int kdw) {
    stg32_nt(r, (uint32_t)key);
    if (kdw == 2) stg32_nt(r + 4, (uint32_t)((uint64_t)key >> 32));
}

// The long-segment path (dml_coalesce_long.hip). `route` is two zeroed device words: the
// number of long segments and the occurrences they hold; `list` has room for n / lmin keys.
struct LongP {
    const uint8_t* values;  // T[n][cols], 4-byte aligned
    const uint32_t* idx;    // occurrence indices, sorted by key, list order inside a key
    const uint32_t* seg;    // seg[u]: the first sorted position of unique key u
    uint8_t* out;           // T[m][cols], 4-byte aligned; REC: the records
    int64_t n, m;
    int64_t rowbytes;
    uint32_t lmin;          // a segment of lmin occurrences and more is long
    uint32_t* list;         // the long keys' u, in no particular order
    uint32_t* route;
    RecP rec;               // REC only
};
// k_co_long_list, then k_co_sum_long or k_co_sum_long_narrow for value type `value_type`;
// `rec`: their record form.
void co_launch_long(const LongP& a, int32_t value_type, bool rec, hipStream_t st);
// k_co_long_list alone: the keys u of [0, m) with lmin occurrences and more, and the route words.
void co_launch_long_list(const uint32_t* seg, int64_t n, int64_t m, uint32_t lmin, uint32_t* list, uint32_t* route,
                         hipStream_t st);

// The element-update sum (dml_coalesce_elems.hip; dml_coalesce_elems_device): occurrence j
// holds `per` (column, delta) pairs, and row / record u of `out` is the dense int32 row of
// key u's elements. `list` and `route` as in LongP.
struct ElemsP {
    const int32_t* cols;  // int32[n][per], 4-byte aligned
    const int32_t* vals;  // int32[n][per], 4-byte aligned
    const uint32_t* idx;  // occurrence indices, sorted by key
    const uint32_t* seg;  // seg[u]: the first sorted position of unique key u
    uint8_t* out;         // int32[m][ncols], 4-byte aligned; REC: the records
    int64_t n, m;
    int64_t rowbytes;     // 4 x ncols
    int64_t nslice;       // co_elems_slices(ncols)
    int32_t ncols, per;
    uint32_t lmin;        // a segment of lmin occurrences and more is long
    uint32_t* list;
    uint32_t* route;
    RecP rec;             // REC only
};
int64_t co_elems_slices(int32_t ncols);
// has_long: k_co_long_list and k_co_elems_long first; then k_co_elems. `rec`: their record form.
void co_launch_elems(const ElemsP& a, bool rec, bool has_long, hipStream_t st);

// ---- the element sum's LDS slice, shared with the element push (dml_push_elems.hip) ----
// Between two phases of a wave's work on its slice: the compiler keeps the LDS operations
// on either side in program order (the hardware runs one wave's in issue order).
__device__ inline void wave_phase() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline void zero_slice(uint32_t* sl, uint32_t w, uint32_t t, uint32_t nt) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (uint32_t v = t; 4 * v < w; v += nt) ((u32x4*)sl)[v] = zero;
}

// One element: sl[col - c0] += val when col lies in [c0, c0 + w). c0 + w <= cols < 2^31, so
// the unsigned difference is under w for exactly those columns, negative ones included.
__device__ inline void add_elem(uint32_t* sl, uint32_t col, uint32_t val, uint32_t c0, uint32_t w) {
    const uint32_t c = col - c0;
    if (c < w) (void)__hip_atomic_fetch_add(sl + c, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Occurrence j's per_occ elements: pairs by 8-byte loads, an odd last one alone.
__device__ inline void add_occ(uint32_t* sl, const ElemsP& a, uint32_t j, uint32_t c0, uint32_t w) {
    const uint32_t* cp = (const uint32_t*)a.cols + (int64_t)j * a.per;
    const uint32_t* vp = (const uint32_t*)a.vals + (int64_t)j * a.per;
    int e = 0;
    for (; e + 2 <= a.per; e += 2) {
        const u32x2 c = ldg8(cp + e), v = ldg8(vp + e);
        add_elem(sl, c.x, v.x, c0, w);
        add_elem(sl, c.y, v.y, c0, w);
    }
    if (e < a.per) add_elem(sl, cp[e], vp[e], c0, w);
}

// ---- an int32 shard slice under the checked add, shared by the element push (dml_push_elems.hip)
// and the compact-row push (dml_compact_rows.hip) ----
constexpr uint32_t kPeNone = 0xFFFFFFFFu;

__device__ inline void stg32(void* p, uint32_t v) { *(DML_GLOBAL uint32_t*)p = v; }

// The wave's lowest `c` (kPeNone: none) as every lane's value.
__device__ inline uint32_t wave_min(uint32_t c) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c = min(c, (uint32_t)__shfl_xor((int)c, d));
    return c;
}

// Vector v of a slice of w dwords at `p`: whole vectors by one 16-byte access, the ragged last
// one's dwords singly.
__device__ inline u32x4 load_vec(const uint8_t* p, uint32_t v, uint32_t w) {
    if (4 * v + 4 <= w) return ldg16(p + 16 * v);
    u32x4 x = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d)
        if (4 * v + d < w) x[d] = ldg32(p + 16 * v + 4 * d);
    return x;
}
__device__ inline void store_vec(uint8_t* p, uint32_t v, uint32_t w, u32x4 x) {
    if (4 * v + 4 <= w) {
        stg16(p + 16 * v, x);
        return;
    }
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d)
        if (4 * v + d < w) stg32(p + 16 * v + 4 * d, x[d]);
}

// Vector v of the item's slice: `sh` is what the shard holds there and `up` the update.
// Apply: sh + up is stored when the update is nonzero, and the lowest dword of the slice whose
// result is negative is kept in `low`. UNDO: `up` is taken back from the dwords whose slice
// position lies above `keep` (the failing element's position in this slice; below zero: all).
template <bool UNDO>
__device__ inline void update_vec(uint8_t* p, uint32_t v, uint32_t w, u32x4 sh, u32x4 up, int64_t keep, uint32_t& low) {
    if (4 * v >= w) return;
    if constexpr (UNDO) {
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if ((int64_t)(4 * v + d) <= keep) up[d] = 0u;
    }
    const u32x4 x = UNDO ? sh - up : sh + up;
    if constexpr (!UNDO) {
#pragma unroll
        for (int d = 3; d >= 0; --d)
            if (4 * v + d < w && (int32_t)x[d] < 0) low = min(low, 4 * v + d);
    }
    if ((up.x | up.y | up.z | up.w) != 0u) store_vec(p, v, w, x);
}

// What an UNDO kernel does with the rows of an item: the failing element (row-major) as (row, col).
struct Undo {
    int64_t row;
    uint32_t col;
};
// The slice positions of shard row `row`, columns [c0, c0 + w), that stay as applied: all (w - 1
// and more) when nothing of the slice is taken back, -1 when everything is.
__device__ inline int64_t undo_keep(const Undo& f, int32_t row, uint32_t c0, uint32_t w) {
    if (row < f.row) return (int64_t)w;
    if (row > f.row) return -1;
    return (int64_t)f.col - (int64_t)c0;
}

// The order stage for keys declared to lie in [first, first + span), 1 <= span <= 2^32
// (dml_coalesce_order.hip; dml_coalescer_set_key_range): kout[i] = key ^ sign bit and
// vout[i] = occurrence index, by key and then by list position, what the library sort leaves.
// `a` and `b` hold n words each and `count` co_order_count_bytes(); none of them is kout or
// vout. A key outside the range makes some thread store `epoch` to *flag; kout and vout are
// then not the order (every access stays in bounds).
struct OrderP {
    const int64_t* keys;
    int64_t n;
    uint64_t first, span;
    uint64_t* a;
    uint64_t* b;
    uint32_t* count;
    uint64_t* kout;
    uint32_t* vout;
    uint32_t* flag;
    uint32_t epoch;
};
// The sum with a store's shard as its sink (dml_push_planes.hip; dml_store_push_planes_device,
// DESIGN.md §4.17): key u's sums are applied to shard row ukeys[u] - first by the store's own
// element update instead of being written anywhere. co_run fills the coalescer's side, the
// store's side comes from its PushSink (dml_internal.h).
struct PushP {
    const uint8_t* values;  // T[n][cols], 4-byte aligned
    const uint32_t* idx;    // occurrence indices, sorted by key, list order inside a key
    const uint32_t* seg;    // seg[u]: the first sorted position of unique key u
    const int64_t* ukeys;   // the distinct keys, ascending
    int64_t n, m;
    int64_t rowbytes;
    int64_t nspan;          // 1-KiB spans of a row
    int32_t lgG;            // log2 of the lanes of a group
    uint32_t lmin;          // a segment of lmin occurrences and more is the long kernels'
    const uint32_t* list;   // the long keys' u (k_co_long_list)
    const uint32_t* route;
    PushSink sink;
    DeltaCand* cand;        // AdaGrad: this launch's candidates, one per block
};
// has_long: k_co_long_list and the long kernels first; then the walk (or its narrow form);
// AdaGrad: the candidates' finalize behind them.
hipError_t launch_push_planes(const PushP& a, int32_t value_type, bool has_long, hipStream_t st);

// The element sum with an int32 store's shard as its sink (dml_push_elems.hip;
// dml_store_push_elems_device). `e.out` and `e.rec` are unused; `e.cols` null:
// the array form.
struct PushElemsP {
    ElemsP e;
    const int64_t* ukeys;  // the distinct keys, ascending
    ElemSink sink;
};
// has_long: k_co_long_list first. The apply kernels, their undo forms, then the verdict.
hipError_t launch_push_elems(const PushElemsP& a, bool has_long, hipStream_t st);

// ---- compact update rows (dml_compact_rows.hip) ----
// The source (dml_coalesce_elems_compact_device): the element sum's inputs in `e` (`e.out` and
// `e.rec` unused), the three entry arrays, and `cnt`, m x nslice + 1 workspace words: the
// count pass leaves the non-zeros of item (u, slice) at cnt[u x nslice + slice], the scan turns
// them into the item's first entry, and the writing pass reads that.
struct CompactP {
    ElemsP e;
    int32_t* ptr;   // int32[m + 1]
    int32_t* ecol;  // int32[nnz]
    int32_t* eval;
    uint32_t* cnt;
};
// has_long: k_co_long_list first. Count (long, short), scan, write (long, short).
void co_launch_compact(const CompactP& a, bool has_long, hipStream_t st);

// The owner's side and the split: PushCompactP, launch_push_compact, launch_compact_split (dml_internal.h).

int co_order_passes(uint64_t span);
size_t co_order_count_bytes();
void co_launch_order(const OrderP& o, hipStream_t st);

}  // namespace dml

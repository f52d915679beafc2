// dml_push_elems.hip — the element push of dml_store_push_elems_device: the
// coalescer's element sum (dml_coalesce_elems.hip, §4.14) with an int32 store's shard as its sink.
//
// A LightLDA worker on the store's own GPU holds token moves: per occurrence a key and per_occ
// (column, delta) pairs. The record route writes the m dense update rows as push records and the
// store's reduce reads them back. Here the order stage and k_co_heads run as they are and the sum
// kernels below end in the store's checked add: per distinct key, ascending, the update row
// u[c] = sum of the key's deltas on column c (mod 2^32), then row[c] += u[c] for every column
// of the row, and every result is checked, those of a zero update included
// (IntMatrixStore.java:171-178). No update row is ever in HBM.
//
//   k_pe_apply<UNDO>       segments under lmin occurrences; k_co_elems' shape. An item is (distinct
//                 key u, slice of kPeSlice dwords of its row); one wave per item with a private
//                 4-KiB LDS slice. Lane 0 loads the key, checks it as a 64-bit value and broadcasts
//                 the shard row (-1: refused, no access). The wave's loads of the shard slice,
//                 kPeVec 16-byte vectors per lane at 4-byte-aligned addresses, are issued before
//                 the walk; the walk is k_co_elems' (zero, ds_add_u32 per element, 64 occurrences
//                 at a time); the slice is read back, added to the held vectors, and only vectors
//                 with a nonzero update are stored. A slice's ragged last vector is loaded and
//                 stored dword by dword: rows under 16 bytes (cols 1 - 3) have no whole vector to
//                 shift back into, and one path serves them all.
//   k_pe_apply_long<UNDO>  keys with lmin occurrences and more (k_co_long_list's list):
//                 k_co_elems_long's block per item, thread t holding vector t of the slice.
//   k_pe_array<UNDO>       IntArrayStore: one wave per distinct key, lanes striding its segment and
//                 summing per_occ values per occurrence, a wave reduction, lane 0 the checked add.
//   k_pe_verdict           one thread, behind them: the call's verdict into the sticky one.
//
// First negative. Inside one call every (row, column) gets exactly one add, so the reference's
// first failing position is the smallest row-major element index whose result is negative. A wave
// that saw a sign bit reduces its lowest such index and reports it by one atomicMin on the call's
// cell. The UNDO instantiations run behind the applies in every call and return at once when the
// cell is untouched; otherwise they rebuild the slices of the rows at and after the failing one
// and subtract them from exactly the elements whose index is greater than the cell's. The
// wrapping subtraction restores those bytes, so the shard holds every add up to and including
// the failing one and none after it, and no copy of it is kept.
//
// A key outside [first, last] is never turned into an address; the lowest such distinct-key index
// goes to `bad`. The keys ascend: ukeys[0] < first stops the record route at its first record, so
// every kernel returns before any store. A negative counter at an in-shard key comes before a key
// above `last` in record order, so k_pe_verdict posts the key verdict only when the cell is
// untouched (collect_apply_check reads the fetch verdict first). A closed sticky verdict, read
// once per kernel, turns the call into a no-op. No float op is in this file.
#include <algorithm>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kPeSlice = DML_COALESCE_ELEMS_SLICE;  // dwords of a row that one item updates
constexpr int kPeWaves = kCoBlock / 64;
constexpr int kPeVec = kPeSlice / 4 / 64;            // 16-byte vectors of a slice per lane
constexpr int kPeLongThreads = 1024;
constexpr int64_t kPeMaxBlocks = (int64_t)1 << 22;
constexpr int kPeLongMaxBlocks = 2048;
static_assert(kPeVec * 256 == kPeSlice && kPeWaves * kPeSlice * 4 <= 65536 && kPeSlice / 4 <= kPeLongThreads,
              "a lane holds whole vectors of its slice; a block's slices fit LDS; a long block covers a slice");

// Nothing of the call is applied: a sticky verdict is closed, or the list's smallest key lies
// below the shard. Block-uniform; every kernel of a call reads the same values, because only
// k_pe_verdict writes them.
__device__ inline bool pe_shut(const PushElemsP& a) {
    return (a.sink.fver->idx != kNoPos) | (*a.sink.neg != kNoPos) | (a.ukeys[0] < a.sink.first);
}
// ... and the last case's report, by one thread of the kernel every call launches.
__device__ inline void pe_report_low(const PushElemsP& a) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.sink.fver->idx == kNoPos && *a.sink.neg == kNoPos &&
        a.ukeys[0] < a.sink.first)
        atomicMin(a.sink.bad, 0ull);
}
// The shard row of distinct key u, -1 refused (reported when `report`).
__device__ inline int32_t pe_row(const PushElemsP& a, int64_t u, bool report) {
    const int64_t key = a.ukeys[u];
    if (key >= a.sink.first && key <= a.sink.last) return (int32_t)(key - a.sink.first);  // rows <= INT32_MAX
    if (report) atomicMin(a.sink.bad, (unsigned long long)u);
    return -1;
}

// wave_min, load_vec / store_vec, update_vec and undo_keep: dml_coalesce_dev.h, shared with the
// compact-row push (dml_compact_rows.hip).

template <bool UNDO>
__global__ __launch_bounds__(kCoBlock) void k_pe_apply(const PushElemsP a) {
    __shared__ u32x4 lds[kPeWaves][kPeSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* sl = (uint32_t*)lds[threadIdx.x >> 6];
    const ElemsP& q = a.e;
    if constexpr (!UNDO) pe_report_low(a);
    if (pe_shut(a)) return;
    Undo f{0, 0};
    if constexpr (UNDO) {
        const unsigned long long cell = *a.sink.cell;
        if (cell == kNoPos) return;
        f.row = (int64_t)(cell / (unsigned long long)a.sink.cols);
        f.col = (uint32_t)(cell % (unsigned long long)a.sink.cols);
    }
    const int64_t nitem = q.m * q.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kPeWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kPeWaves) {
        const int64_t u = q.nslice == 1 ? item : item / q.nslice;
        const uint32_t c0 = (uint32_t)(item - u * q.nslice) * kPeSlice;
        const uint32_t w = (uint32_t)q.ncols - c0 < (uint32_t)kPeSlice ? (uint32_t)q.ncols - c0 : (uint32_t)kPeSlice;
        const uint32_t s = q.seg[u], e = u + 1 < q.m ? q.seg[u + 1] : (uint32_t)q.n;
        if (e - s >= q.lmin) continue;  // the long route's
        int32_t mine = -1;
        if (lane == 0) mine = pe_row(a, u, !UNDO && c0 == 0);
        const int32_t row = __builtin_amdgcn_readfirstlane(mine);
        if (row < 0) continue;
        int64_t keep = -1;
        if constexpr (UNDO) {
            keep = undo_keep(f, row, c0, w);
            if (keep >= (int64_t)w - 1) continue;
        }
        uint8_t* p = (uint8_t*)a.sink.data + ((int64_t)row * q.ncols + c0) * 4;
        u32x4 sh[kPeVec];  // in flight over the walk
#pragma unroll
        for (int k = 0; k < kPeVec; ++k) {
            const uint32_t v = lane + 64 * k;
            sh[k] = u32x4{0u, 0u, 0u, 0u};
            if (4 * v < w) sh[k] = load_vec(p, v, w);
        }
        uint32_t j = s + lane < e ? q.idx[s + lane] : 0u;
        zero_slice(sl, w, lane, 64);
        wave_phase();
        for (uint32_t base = s; base < e; base += 64) {
            const uint32_t pn = base + 64 + lane;
            const uint32_t jn = pn < e ? q.idx[pn] : 0u;  // in flight over this batch's atomics
            if (base + lane < e) add_occ(sl, q, j, c0, w);
            j = jn;
        }
        wave_phase();
        uint32_t low = kPeNone;
#pragma unroll
        for (int k = 0; k < kPeVec; ++k) {
            const uint32_t v = lane + 64 * k;
            const u32x4 up = 4 * v < w ? ((const u32x4*)sl)[v] : u32x4{0u, 0u, 0u, 0u};
            update_vec<UNDO>(p, v, w, sh[k], up, keep, low);
        }
        if constexpr (!UNDO) {
            if (__ballot(low != kPeNone) != 0ull) {  // rare: the wave's lowest failing column
                low = wave_min(low);
                if (lane == 0) atomicMin(a.sink.cell, (unsigned long long)((int64_t)row * q.ncols + c0 + low));
            }
        }
        wave_phase();  // the next item's zeroing comes after this read-back
    }
}

template <bool UNDO>
__global__ __launch_bounds__(kPeLongThreads) void k_pe_apply_long(const PushElemsP a) {
    __shared__ u32x4 lds[kPeSlice / 4];
    const uint32_t t = threadIdx.x;
    uint32_t* sl = (uint32_t*)lds;
    const ElemsP& q = a.e;
    if (pe_shut(a)) return;
    Undo f{0, 0};
    if constexpr (UNDO) {
        const unsigned long long cell = *a.sink.cell;
        if (cell == kNoPos) return;
        f.row = (int64_t)(cell / (unsigned long long)a.sink.cols);
        f.col = (uint32_t)(cell % (unsigned long long)a.sink.cols);
    }
    const int64_t nitem = (int64_t)q.route[0] * q.nslice;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t u = q.list[item / q.nslice];
        const uint32_t c0 = (uint32_t)(item % q.nslice) * kPeSlice;
        const uint32_t w = (uint32_t)q.ncols - c0 < (uint32_t)kPeSlice ? (uint32_t)q.ncols - c0 : (uint32_t)kPeSlice;
        const int32_t row = pe_row(a, u, !UNDO && t == 0 && c0 == 0);  // block-uniform
        if (row < 0) continue;
        int64_t keep = -1;
        if constexpr (UNDO) {
            keep = undo_keep(f, row, c0, w);
            if (keep >= (int64_t)w - 1) continue;
        }
        const uint32_t s = q.seg[u], e = u + 1 < q.m ? q.seg[u + 1] : (uint32_t)q.n;
        uint8_t* p = (uint8_t*)a.sink.data + ((int64_t)row * q.ncols + c0) * 4;
        u32x4 sh = {0u, 0u, 0u, 0u};  // thread t's vector of the shard slice, in flight over the segment
        if (4 * t < w) sh = load_vec(p, t, w);
        uint32_t j = s + t < e ? q.idx[s + t] : 0u;
        zero_slice(sl, w, t, kPeLongThreads);
        __syncthreads();
        for (uint32_t base = s; base < e; base += kPeLongThreads) {
            const uint32_t pn = base + kPeLongThreads + t;
            const uint32_t jn = pn < e ? q.idx[pn] : 0u;
            if (base + t < e) add_occ(sl, q, j, c0, w);
            j = jn;
        }
        __syncthreads();
        uint32_t low = kPeNone;
        if (4 * t < w) update_vec<UNDO>(p, t, w, sh, ((const u32x4*)sl)[t], keep, low);
        if constexpr (!UNDO) {
            if (__ballot(low != kPeNone) != 0ull) {  // wave-uniform; one report per wave that saw one
                low = wave_min(low);
                if ((t & 63) == 0) atomicMin(a.sink.cell, (unsigned long long)((int64_t)row * q.ncols + c0 + low));
            }
        }
        __syncthreads();  // the next item's zeroing comes after every thread's read-back
    }
}

// IntArrayStore: the key's one counter takes every element of its occurrences. int32 adds wrap and
// commute, so the lanes' partial sums combine in any order.
template <bool UNDO>
__global__ __launch_bounds__(kCoBlock) void k_pe_array(const PushElemsP a) {
    const uint32_t lane = threadIdx.x & 63;
    const ElemsP& q = a.e;
    if constexpr (!UNDO) pe_report_low(a);
    if (pe_shut(a)) return;
    unsigned long long cell = kNoPos;
    if constexpr (UNDO) {
        cell = *a.sink.cell;
        if (cell == kNoPos) return;
    }
    for (int64_t u = (int64_t)blockIdx.x * kPeWaves + (threadIdx.x >> 6); u < q.m; u += (int64_t)gridDim.x * kPeWaves) {
        int32_t mine = -1;
        if (lane == 0) mine = pe_row(a, u, !UNDO);
        const int32_t row = __builtin_amdgcn_readfirstlane(mine);
        if (row < 0) continue;
        if constexpr (UNDO) {
            if ((unsigned long long)row <= cell) continue;  // applied up to and including the failing add
        }
        uint32_t sh = 0;
        if (lane == 0) sh = ldg32((const uint8_t*)(a.sink.data + row));  // in flight over the segment
        const uint32_t s = q.seg[u], e = u + 1 < q.m ? q.seg[u + 1] : (uint32_t)q.n;
        uint32_t sum = 0;
        for (uint32_t pos = s + lane; pos < e; pos += 64) {
            const uint32_t* vp = (const uint32_t*)q.vals + (int64_t)q.idx[pos] * q.per;
            for (int k = 0; k < q.per; ++k) sum += vp[k];
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d);
        if (lane == 0) {
            const uint32_t x = UNDO ? sh - sum : sh + sum;
            if (sum != 0u) stg32(a.sink.data + row, x);
            if constexpr (!UNDO) {
                if ((int32_t)x < 0) atomicMin(a.sink.cell, (unsigned long long)row);
            }
        }
    }
}

// Behind a call's kernels: its verdict into the sticky one that record order puts first, both
// per-call cells reset. A shut call touched neither cell.
__global__ void k_pe_verdict(const PushElemsP a) {
    const ElemSink& k = a.sink;
    const unsigned long long cell = *k.cell, bad = *k.bad;
    if (cell != kNoPos) {
        if (*k.neg == kNoPos) *k.neg = cell;
    } else if (bad != kNoPos && k.fver->idx == kNoPos) {
        k.fver->key = a.ukeys[bad];
        k.fver->idx = bad;
    }
    *k.cell = kNoPos;
    *k.bad = kNoPos;
}

template <bool UNDO>
void launch_pass(const PushElemsP& a, bool has_long, hipStream_t st) {
    const ElemsP& q = a.e;
    if (!q.cols) {
        const int64_t blocks = std::min<int64_t>((q.m + kPeWaves - 1) / kPeWaves, kPeMaxBlocks);
        hipLaunchKernelGGL((k_pe_array<UNDO>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
        return;
    }
    if (has_long) {  // the blocks read the list's count; its capacity bounds the grid
        const unsigned grid = (unsigned)std::min<int64_t>(q.n / q.lmin * q.nslice, kPeLongMaxBlocks);
        hipLaunchKernelGGL((k_pe_apply_long<UNDO>), dim3(grid), dim3(kPeLongThreads), 0, st, a);
    }
    const int64_t nitem = q.m * q.nslice;
    const int64_t blocks = std::min<int64_t>((nitem + kPeWaves - 1) / kPeWaves, kPeMaxBlocks);
    hipLaunchKernelGGL((k_pe_apply<UNDO>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
}

}  // namespace

hipError_t launch_push_elems(const PushElemsP& a, bool has_long, hipStream_t st) {
    has_long = has_long && a.e.cols;  // the array kernel walks every segment itself
    if (has_long) co_launch_long_list(a.e.seg, a.e.n, a.e.m, a.e.lmin, a.e.list, a.e.route, st);
    launch_pass<false>(a, has_long, st);
    launch_pass<true>(a, has_long, st);
    hipLaunchKernelGGL(k_pe_verdict, dim3(1), dim3(1), 0, st, a);
    return hipGetLastError();
}

}  // namespace dml

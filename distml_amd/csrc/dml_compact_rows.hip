// dml_compact_rows.hip — compact int32 update rows: the form in which a LightLDA
// worker's element updates leave its rank. A compact row list is the distinct keys ascending
// (int64[m]), ptr (int32[m + 1]) and per key the non-zero (column, value) entries of its summed
// update row (ecol, eval: int32[nnz]), columns ascending. A dense update record is 4 x cols bytes
// per word however few topics its tokens touched; a compact row is 8 bytes per touched topic.
//
// Source (dml_coalesce_elems_compact_device), behind the coalescer's order stage and k_co_heads:
//   k_cr_src<false>       the count pass. k_co_elems' shape: an item is (distinct key u, slice of
//                 kCrSlice dwords of its row), one wave per item with a private 4-KiB LDS slice;
//                 zero, one ds_add_u32 per element 64 occurrences at a time. Then the slice is
//                 read back 64 dwords a round and the ballots' popcounts add up to the item's
//                 non-zeros, cnt[item].
//   k_cr_src_long<false>  keys of lmin occurrences and more (k_co_long_list's list): a block of
//                 kCrLongThreads threads per item, thread t holding dword t of the slice, so a
//                 wave is one round; the 16 waves' popcounts meet in LDS.
//   k_cr_scan     one block: cnt[] to its exclusive running sum, 4 counts per thread and tiles of
//                 4096 carried forward; ptr[u] = the sum in front of key u's first slice,
//                 ptr[m] = cnt[m x nslice] = nnz. The compact fetch (dml_fetch_compact.hip) runs
//                 it too, through launch_compact_scan.
//   k_cr_src<true>, k_cr_src_long<true>   the writing pass. The slice is REBUILT, not kept: kept
//                 slices are the dense plane (m x 4 x cols bytes written and read back, 262 MB at
//                 config 5), rebuilt ones cost a second read of the elements (16 MB there). Per
//                 round, lane l's non-zero dword goes to cnt[item] + (non-zeros of the rounds
//                 before) + popcount(ballot below l): a position is a sum of counts, no atomic
//                 decides one, so two runs give equal bytes and a key's columns ascend across
//                 slices and rounds.
//
// Owner (dml_store_push_compact_rows_device), all on the store's apply stream, no host wait:
//   k_cr_check    ptr[0] == 0, ptr non-decreasing, keys strictly ascending: the lowest faulty index
//                 by atomicMin into the call's `form` cell, which every later kernel reads before
//                 anything else (a malformed list is never walked). It also lists the keys with
//                 kCrLongEntries entries and more (one atomic on `route`; no byte depends on the
//                 list's order) and reports a smallest key below the shard.
//   k_cr_apply<UNDO>       one wave per (key, slice) with fewer entries: k_pe_apply with the
//                 walk over the key's entries (ecol, eval 64 at a time) in place of occurrences.
//                 The shard slice's 16-byte loads are issued first; zero, LDS adds, read back,
//                 add, check every dword, store the vectors whose update is non-zero.
//   k_cr_apply_long<UNDO>  the listed keys: a block per (key, slice), thread t holding vector t.
//   k_cr_verdict  one thread: form, then the first negative counter, then the lowest key outside
//                 the shard, into the store's sticky verdicts; the call's cells reset.
// First negative, UNDO, key range and a closed verdict are §4.18's (dml_push_elems.hip).
//
// dml_compact_rows_split: k_cr_split (a binary search per owner boundary) and k_cr_rebase.
// No float op is in this file.
#include <algorithm>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kCrSlice = DML_COALESCE_ELEMS_SLICE;  // dwords of a row that one item holds
constexpr int kCrWaves = kCoBlock / 64;
constexpr int kCrVec = kCrSlice / 4 / 64;            // 16-byte vectors of a slice per lane
constexpr int kCrLongThreads = 1024;
constexpr int kCrLongWaves = kCrLongThreads / 64;
constexpr int kCrScanPer = 4;                        // counts per thread of k_cr_scan
constexpr int64_t kCrMaxBlocks = (int64_t)1 << 22;
constexpr int kCrLongMaxBlocks = 2048;
constexpr int kCrOwnerLongBlocks = 256;              // the owner cannot know the list's length
constexpr uint32_t kCrLongEntries = DML_COMPACT_ROWS_LONG_ENTRIES;
static_assert(kCrVec * 256 == kCrSlice && kCrWaves * kCrSlice * 4 <= 65536 && kCrSlice == kCrLongThreads,
              "a lane holds whole vectors of its slice; a block's slices fit LDS; a long block's thread is a dword");

// ---------------------------------------------------------------- source

// Rounds of 64 dwords over the slice's w: returns `base` + the non-zeros; WRITE stores each at
// base + the non-zeros before it.
template <bool WRITE>
__device__ inline uint32_t squeeze(const uint32_t* sl, uint32_t w, uint32_t c0, uint32_t lane, uint32_t base,
                                   int32_t* ecol, int32_t* eval) {
    for (uint32_t d0 = 0; d0 < w; d0 += 64) {
        const uint32_t d = d0 + lane;
        const uint32_t v = d < w ? sl[d] : 0u;
        const unsigned long long nz = __ballot(v != 0u);
        if constexpr (WRITE) {
            if (v != 0u) {
                const uint32_t pos = base + (uint32_t)__popcll(nz & ((1ull << lane) - 1ull));
                stg32_nt(ecol + pos, c0 + d);
                stg32_nt(eval + pos, v);
            }
        }
        base += (uint32_t)__popcll(nz);
    }
    return base;
}

template <bool WRITE>
__global__ __launch_bounds__(kCoBlock) void k_cr_src(const CompactP a) {
    __shared__ u32x4 lds[kCrWaves][kCrSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* sl = (uint32_t*)lds[threadIdx.x >> 6];
    const ElemsP& q = a.e;
    const int64_t nitem = q.m * q.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kCrWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kCrWaves) {
        const int64_t u = q.nslice == 1 ? item : item / q.nslice;
        const uint32_t c0 = (uint32_t)(item - u * q.nslice) * kCrSlice;
        const uint32_t w = (uint32_t)q.ncols - c0 < (uint32_t)kCrSlice ? (uint32_t)q.ncols - c0 : (uint32_t)kCrSlice;
        const uint32_t s = q.seg[u], e = u + 1 < q.m ? q.seg[u + 1] : (uint32_t)q.n;
        if (e - s >= q.lmin) continue;  // the long route's
        uint32_t base = 0;
        if constexpr (WRITE) base = a.cnt[item];  // in flight over the walk
        uint32_t j = s + lane < e ? q.idx[s + lane] : 0u;
        zero_slice(sl, w, lane, 64);
        wave_phase();
        for (uint32_t b = s; b < e; b += 64) {
            const uint32_t pn = b + 64 + lane;
            const uint32_t jn = pn < e ? q.idx[pn] : 0u;  // in flight over this batch's atomics
            if (b + lane < e) add_occ(sl, q, j, c0, w);
            j = jn;
        }
        wave_phase();
        const uint32_t end = squeeze<WRITE>(sl, w, c0, lane, base, a.ecol, a.eval);
        if constexpr (!WRITE) {
            if (lane == 0) a.cnt[item] = end;
        }
        wave_phase();  // the next item's zeroing comes after this read-back
    }
}

template <bool WRITE>
__global__ __launch_bounds__(kCrLongThreads) void k_cr_src_long(const CompactP a) {
    __shared__ u32x4 lds[kCrSlice / 4];
    __shared__ uint32_t wcnt[kCrLongWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t* sl = (uint32_t*)lds;
    const ElemsP& q = a.e;
    const int64_t nitem = (int64_t)q.route[0] * q.nslice;
    for (int64_t it = blockIdx.x; it < nitem; it += gridDim.x) {
        const int64_t u = q.list[it / q.nslice];
        const int64_t item = u * q.nslice + it % q.nslice;
        const uint32_t c0 = (uint32_t)(it % q.nslice) * kCrSlice;
        const uint32_t w = (uint32_t)q.ncols - c0 < (uint32_t)kCrSlice ? (uint32_t)q.ncols - c0 : (uint32_t)kCrSlice;
        const uint32_t s = q.seg[u], e = u + 1 < q.m ? q.seg[u + 1] : (uint32_t)q.n;
        uint32_t base = 0;
        if constexpr (WRITE) base = a.cnt[item];
        uint32_t j = s + t < e ? q.idx[s + t] : 0u;
        zero_slice(sl, w, t, kCrLongThreads);
        __syncthreads();
        for (uint32_t b = s; b < e; b += kCrLongThreads) {
            const uint32_t pn = b + kCrLongThreads + t;
            const uint32_t jn = pn < e ? q.idx[pn] : 0u;
            if (b + t < e) add_occ(sl, q, j, c0, w);
            j = jn;
        }
        __syncthreads();
        const uint32_t v = t < w ? sl[t] : 0u;  // wave `wave` is round `wave` of the slice
        const unsigned long long nz = __ballot(v != 0u);
        if (lane == 0) wcnt[wave] = (uint32_t)__popcll(nz);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kCrLongWaves; ++k) {
            if (k < (int)wave) before += wcnt[k];
            all += wcnt[k];
        }
        if constexpr (WRITE) {
            if (v != 0u) {
                const uint32_t pos = base + before + (uint32_t)__popcll(nz & ((1ull << lane) - 1ull));
                stg32_nt(a.ecol + pos, c0 + t);
                stg32_nt(a.eval + pos, v);
            }
        } else {
            if (t == 0) a.cnt[item] = all;
        }
        __syncthreads();  // the next item's zeroing and counts come after every thread's read
    }
}

// One block. cnt[0 .. nitem) from counts to the exclusive running sum, cnt[nitem] = the total;
// ptr[u] = cnt[u x nslice], ptr[m] = the total.
__global__ __launch_bounds__(kCrLongThreads) void k_cr_scan(uint32_t* __restrict__ cnt, int64_t nitem, int64_t nslice,
                                                           int32_t* __restrict__ ptr) {
    __shared__ uint32_t wsum[kCrLongWaves];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t carry = 0;
    for (int64_t tile = 0; tile < nitem; tile += kCrLongThreads * kCrScanPer) {
        const int64_t i0 = tile + (int64_t)t * kCrScanPer;
        uint32_t v[kCrScanPer], mine = 0;
#pragma unroll
        for (int k = 0; k < kCrScanPer; ++k) {
            v[k] = i0 + k < nitem ? cnt[i0 + k] : 0u;
            mine += v[k];
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t x = __shfl_up(incl, d);
            if ((int)lane >= d) incl += x;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kCrLongWaves; ++k) {
            if (k < (int)wave) before += wsum[k];
            all += wsum[k];
        }
        uint32_t run = carry + before + incl - mine;
#pragma unroll
        for (int k = 0; k < kCrScanPer; ++k) {
            const int64_t i = i0 + k;
            if (i < nitem) {
                cnt[i] = run;
                if (nslice == 1) ptr[i] = (int32_t)run;
                else if (i % nslice == 0) ptr[i / nslice] = (int32_t)run;
            }
            run += v[k];
        }
        carry += all;
        __syncthreads();  // wsum is rewritten by the next tile
    }
    if (t == 0) {
        cnt[nitem] = carry;
        ptr[nitem / nslice] = (int32_t)carry;
    }
}

template <bool WRITE>
void launch_src(const CompactP& a, bool has_long, hipStream_t st) {
    const ElemsP& q = a.e;
    if (has_long) {  // the list's capacity bounds the grid; the blocks read the count
        const unsigned grid = (unsigned)std::min<int64_t>(q.n / q.lmin * q.nslice, kCrLongMaxBlocks);
        hipLaunchKernelGGL((k_cr_src_long<WRITE>), dim3(grid), dim3(kCrLongThreads), 0, st, a);
    }
    const int64_t nitem = q.m * q.nslice;
    const int64_t blocks = std::min<int64_t>((nitem + kCrWaves - 1) / kCrWaves, kCrMaxBlocks);
    hipLaunchKernelGGL((k_cr_src<WRITE>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
}

// ---------------------------------------------------------------- owner

// Nothing of the call is applied: a sticky verdict is closed, the list is malformed, or its
// smallest key lies below the shard. Block-uniform; the apply kernels of a call read the same
// values, because only k_cr_check (before them) and k_cr_verdict (behind them) write these.
__device__ inline bool cr_shut(const PushCompactP& a) {
    if ((a.sink.fver->idx != kNoPos) | (*a.sink.neg != kNoPos) | (*a.form != kNoPos)) return true;
    return a.keys[0] < a.sink.first;  // read only once the list is known to be well formed
}
// The shard row of key u, -1 refused (reported when `report`).
__device__ inline int32_t cr_row(const PushCompactP& a, int64_t u, bool report) {
    const int64_t key = a.keys[u];
    if (key >= a.sink.first && key <= a.sink.last) return (int32_t)(key - a.sink.first);  // rows <= INT32_MAX
    if (report) atomicMin(a.sink.bad, (unsigned long long)u);
    return -1;
}

__global__ __launch_bounds__(kCoBlock) void k_cr_check(const PushCompactP a) {
    if ((a.sink.fver->idx != kNoPos) | (*a.sink.neg != kNoPos)) return;  // a shut call touches no cell
    for (int64_t u = (int64_t)blockIdx.x * kCoBlock + threadIdx.x; u < a.m; u += (int64_t)gridDim.x * kCoBlock) {
        const int32_t p0 = a.ptr[u], p1 = a.ptr[u + 1];
        const bool pf = p1 < p0 || (u == 0 && p0 != 0);
        const bool kf = u > 0 && a.keys[u] <= a.keys[u - 1];
        if (kf | pf) atomicMin(a.form, 2ull * (unsigned long long)u + (kf ? 0ull : 1ull));
        else if ((uint32_t)(p1 - p0) >= kCrLongEntries) a.list[atomicAdd(a.route, 1u)] = (uint32_t)u;  // at most m
        if (u == 0 && a.keys[0] < a.sink.first) atomicMin(a.sink.bad, 0ull);
    }
}

template <bool UNDO>
__global__ __launch_bounds__(kCoBlock) void k_cr_apply(const PushCompactP a) {
    __shared__ u32x4 lds[kCrWaves][kCrSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* sl = (uint32_t*)lds[threadIdx.x >> 6];
    if (cr_shut(a)) return;
    Undo f{0, 0};
    if constexpr (UNDO) {
        const unsigned long long cell = *a.sink.cell;
        if (cell == kNoPos) return;
        f.row = (int64_t)(cell / (unsigned long long)a.sink.cols);
        f.col = (uint32_t)(cell % (unsigned long long)a.sink.cols);
    }
    const int64_t nitem = a.m * a.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kCrWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kCrWaves) {
        const int64_t u = a.nslice == 1 ? item : item / a.nslice;
        const uint32_t c0 = (uint32_t)(item - u * a.nslice) * kCrSlice;
        const uint32_t w = (uint32_t)a.ncols - c0 < (uint32_t)kCrSlice ? (uint32_t)a.ncols - c0 : (uint32_t)kCrSlice;
        const uint32_t s = (uint32_t)a.ptr[u], e = (uint32_t)a.ptr[u + 1];
        if (e - s >= kCrLongEntries) continue;  // the block route's
        int32_t mine = -1;
        if (lane == 0) mine = cr_row(a, u, !UNDO && c0 == 0);
        const int32_t row = __builtin_amdgcn_readfirstlane(mine);
        if (row < 0) continue;
        int64_t keep = -1;
        if constexpr (UNDO) {
            keep = undo_keep(f, row, c0, w);
            if (keep >= (int64_t)w - 1) continue;
        }
        uint8_t* p = (uint8_t*)a.sink.data + ((int64_t)row * a.ncols + c0) * 4;
        u32x4 sh[kCrVec];  // in flight over the walk
#pragma unroll
        for (int k = 0; k < kCrVec; ++k) {
            const uint32_t v = lane + 64 * k;
            sh[k] = u32x4{0u, 0u, 0u, 0u};
            if (4 * v < w) sh[k] = load_vec(p, v, w);
        }
        uint32_t ec = 0, ev = 0;
        if (s + lane < e) {
            ec = (uint32_t)a.ecol[s + lane];
            ev = (uint32_t)a.eval[s + lane];
        }
        zero_slice(sl, w, lane, 64);
        wave_phase();
        for (uint32_t b = s; b < e; b += 64) {
            const uint32_t pn = b + 64 + lane;
            uint32_t cn = 0, vn = 0;
            if (pn < e) {  // in flight over this batch's atomics
                cn = (uint32_t)a.ecol[pn];
                vn = (uint32_t)a.eval[pn];
            }
            if (b + lane < e) add_elem(sl, ec, ev, c0, w);
            ec = cn;
            ev = vn;
        }
        wave_phase();
        uint32_t low = kPeNone;
#pragma unroll
        for (int k = 0; k < kCrVec; ++k) {
            const uint32_t v = lane + 64 * k;
            const u32x4 up = 4 * v < w ? ((const u32x4*)sl)[v] : u32x4{0u, 0u, 0u, 0u};
            update_vec<UNDO>(p, v, w, sh[k], up, keep, low);
        }
        if constexpr (!UNDO) {
            if (__ballot(low != kPeNone) != 0ull) {  // rare: the wave's lowest failing column
                low = wave_min(low);
                if (lane == 0) atomicMin(a.sink.cell, (unsigned long long)((int64_t)row * a.ncols + c0 + low));
            }
        }
        wave_phase();  // the next item's zeroing comes after this read-back
    }
}

template <bool UNDO>
__global__ __launch_bounds__(kCrLongThreads) void k_cr_apply_long(const PushCompactP a) {
    __shared__ u32x4 lds[kCrSlice / 4];
    const uint32_t t = threadIdx.x;
    uint32_t* sl = (uint32_t*)lds;
    if (cr_shut(a)) return;
    Undo f{0, 0};
    if constexpr (UNDO) {
        const unsigned long long cell = *a.sink.cell;
        if (cell == kNoPos) return;
        f.row = (int64_t)(cell / (unsigned long long)a.sink.cols);
        f.col = (uint32_t)(cell % (unsigned long long)a.sink.cols);
    }
    const int64_t nitem = (int64_t)a.route[0] * a.nslice;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t u = a.list[item / a.nslice];
        const uint32_t c0 = (uint32_t)(item % a.nslice) * kCrSlice;
        const uint32_t w = (uint32_t)a.ncols - c0 < (uint32_t)kCrSlice ? (uint32_t)a.ncols - c0 : (uint32_t)kCrSlice;
        const int32_t row = cr_row(a, u, !UNDO && t == 0 && c0 == 0);  // block-uniform
        if (row < 0) continue;
        int64_t keep = -1;
        if constexpr (UNDO) {
            keep = undo_keep(f, row, c0, w);
            if (keep >= (int64_t)w - 1) continue;
        }
        const uint32_t s = (uint32_t)a.ptr[u], e = (uint32_t)a.ptr[u + 1];
        uint8_t* p = (uint8_t*)a.sink.data + ((int64_t)row * a.ncols + c0) * 4;
        u32x4 sh = {0u, 0u, 0u, 0u};  // thread t's vector of the shard slice, in flight over the entries
        if (4 * t < w) sh = load_vec(p, t, w);
        zero_slice(sl, w, t, kCrLongThreads);
        __syncthreads();
        for (uint32_t pos = s + t; pos < e; pos += kCrLongThreads)
            add_elem(sl, (uint32_t)a.ecol[pos], (uint32_t)a.eval[pos], c0, w);
        __syncthreads();
        uint32_t low = kPeNone;
        if (4 * t < w) update_vec<UNDO>(p, t, w, sh, ((const u32x4*)sl)[t], keep, low);
        if constexpr (!UNDO) {
            if (__ballot(low != kPeNone) != 0ull) {  // wave-uniform; one report per wave that saw one
                low = wave_min(low);
                if ((t & 63) == 0) atomicMin(a.sink.cell, (unsigned long long)((int64_t)row * a.ncols + c0 + low));
            }
        }
        __syncthreads();  // the next item's zeroing comes after every thread's read-back
    }
}

// Behind a call's kernels: its verdict into the sticky one that record order puts first (a
// malformed list was never a push: it comes before both), the call's cells reset. A call shut
// by a closed sticky verdict touched no cell.
__global__ void k_cr_verdict(const PushCompactP a) {
    const ElemSink& k = a.sink;
    const unsigned long long cell = *k.cell, bad = *k.bad, form = *a.form;
    if (form != kNoPos) {
        if (k.fver->idx == kNoPos && *k.neg == kNoPos) {
            k.fver->key = (form & 1ull) ? -1 : a.keys[form >> 1];
            k.fver->idx = kVerdictMalformed;
        }
    } else if (cell != kNoPos) {
        if (*k.neg == kNoPos) *k.neg = cell;
    } else if (bad != kNoPos && k.fver->idx == kNoPos) {
        k.fver->key = a.keys[bad];
        k.fver->idx = bad;
    }
    *k.cell = kNoPos;
    *k.bad = kNoPos;
    *a.form = kNoPos;
    *a.route = 0u;
}

template <bool UNDO>
void launch_apply(const PushCompactP& a, hipStream_t st) {
    const int64_t nitem = a.m * a.nslice;
    const unsigned lgrid = (unsigned)std::min<int64_t>(nitem, kCrOwnerLongBlocks);
    hipLaunchKernelGGL((k_cr_apply_long<UNDO>), dim3(lgrid), dim3(kCrLongThreads), 0, st, a);
    const int64_t blocks = std::min<int64_t>((nitem + kCrWaves - 1) / kCrWaves, kCrMaxBlocks);
    hipLaunchKernelGGL((k_cr_apply<UNDO>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
}

// ---------------------------------------------------------------- split

// Thread q <= world: the first row at or above owner q's first key under
// KeyRange.linearSplit(world) of [0, total_rows) (q == world: total_rows), and its first entry.
__global__ void k_cr_split(const int64_t* __restrict__ keys, int64_t m, const int32_t* __restrict__ ptr,
                           int64_t total_rows, int32_t world, int64_t* __restrict__ row_off,
                           int64_t* __restrict__ entry_off) {
    const int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q > world) return;
    const int64_t step = (total_rows - 1 + world) / world;  // KeyRange.java:68-80 with first 0
    const int64_t bound = (int64_t)q * step < total_rows ? (int64_t)q * step : total_rows;
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < bound) lo = mid + 1;
        else hi = mid;
    }
    row_off[q] = lo;
    entry_off[q] = ptr[lo];
}

// Owner blockIdx.y's slice of ptr, rebased to start at 0, at ptr_out[row_off[q] + q ...]: its
// rows + 1 words, so the slices of all owners lie back to back in m + world words.
__global__ __launch_bounds__(kCoBlock) void k_cr_rebase(const int32_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ row_off,
                                                        int32_t* __restrict__ ptr_out) {
    const int64_t q = blockIdx.y;
    const int64_t r0 = row_off[q], r1 = row_off[q + 1];
    const int32_t base = ptr[r0];
    for (int64_t i = r0 + (int64_t)blockIdx.x * kCoBlock + threadIdx.x; i <= r1; i += (int64_t)gridDim.x * kCoBlock)
        ptr_out[i + q] = ptr[i] - base;
}

}  // namespace

void launch_compact_scan(uint32_t* cnt, int64_t nitem, int64_t nslice, int32_t* ptr, hipStream_t st) {
    hipLaunchKernelGGL(k_cr_scan, dim3(1), dim3(kCrLongThreads), 0, st, cnt, nitem, nslice, ptr);
}

void co_launch_compact(const CompactP& a, bool has_long, hipStream_t st) {
    const ElemsP& q = a.e;
    if (has_long) co_launch_long_list(q.seg, q.n, q.m, q.lmin, q.list, q.route, st);
    launch_src<false>(a, has_long, st);
    launch_compact_scan(a.cnt, q.m * q.nslice, q.nslice, a.ptr, st);
    launch_src<true>(a, has_long, st);
}

hipError_t launch_push_compact(const PushCompactP& a, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>((a.m + kCoBlock - 1) / kCoBlock, 1024);
    hipLaunchKernelGGL(k_cr_check, dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
    launch_apply<false>(a, st);
    launch_apply<true>(a, st);
    hipLaunchKernelGGL(k_cr_verdict, dim3(1), dim3(1), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_compact_split(const int64_t* keys, int64_t m, const int32_t* ptr, int64_t total_rows, int32_t world,
                                int64_t* row_off, int64_t* entry_off, int32_t* ptr_out, hipStream_t st) {
    hipLaunchKernelGGL(k_cr_split, dim3((unsigned)(world + 1 + 63) / 64), dim3(64), 0, st, keys, m, ptr, total_rows,
                       world, row_off, entry_off);
    const int64_t per = (m + world) / world + 1;  // blocks sized for an even split; the loop covers the rest
    const unsigned gx = (unsigned)std::min<int64_t>((per + kCoBlock - 1) / kCoBlock, 1024);
    hipLaunchKernelGGL(k_cr_rebase, dim3(gx, (unsigned)world), dim3(kCoBlock), 0, st, ptr, row_off, ptr_out);
    return hipGetLastError();
}

}  // namespace dml

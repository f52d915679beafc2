// dml_compact_rows_batch.hip — a batch of compact int32 update rows in one pass over the shard
// (DESIGN.md §4.21): the owner's end of a group step, where every source rank's run of summed
// LightLDA updates (dml_compact_rows.hip, §4.19) lies in a receive slab. The store ends byte for
// byte where the runs' successive single calls leave it, but a shard row that several runs list is
// read once and written once, and the whole batch is five launches.
//
// The run table (at most DML_COMPACT_ROWS_BATCH_MAX_RUNS = 64 runs: four pointers each, and the
// running sum of their row counts) travels in the kernel arguments. 64 is also the width of a
// wave: lane q of a wave stands for run q wherever the runs are looked at side by side.
//
//   k_crb_check   one thread per (run, row): the single call's form checks into the run's `form`
//                 cell and the lowest key outside the shard into its `bad` cell (2 x index, + 1 for
//                 a key above `last`: an ascending run with a key below `first` leaves 0).
//   k_crb_stop    one wave, lane q reading run q's cells: the first run with a fault is the
//                 batch's stop, and `nwalk` the number of runs that apply anything: stop when it is
//                 malformed or starts below the shard, stop + 1 when it only reaches above it.
//                 Every later kernel reads that word first; runs at and behind nwalk are never
//                 walked or searched. A batch behind a closed verdict gets nwalk 0.
//   k_crb_apply<UNDO>   an item is (run r, row i, slice of kCrbSlice dwords), one wave per item.
//                 Lane q binary-searches the item's key in run q (all runs at once, one pass of
//                 dependent loads), and the ballot of the hits is the set of runs that list the
//                 key. Its lowest bit owns the row: a wave whose r is not that bit leaves. No sort
//                 and no atomic decides ownership, because each run is strictly ascending. The
//                 owner loads the shard slice by 16-byte loads into registers, then per listed run
//                 in run order: zero its 4-KiB LDS slice, one ds_add_u32 per entry 64 at a time with
//                 the next 64 in flight, read the slice back, add it to the registers, check every
//                 dword. A negative one becomes the order word (run x rows + row) x cols + col, the
//                 wave's lowest by one atomicMin. The slice is stored once, the vectors some run
//                 changed. A row of any entry count takes this route (no block route: §4.21).
//                 UNDO: returns at once when no order word was recorded; else the same walk over
//                 the runs from the failing one on sums what lies behind the failing order word
//                 and takes it back in one load and one store.
//   k_crb_verdict one wave: the first negative counter, else stop's fault, into the store's sticky
//                 verdicts as the single call's k_cr_verdict writes them; the call's cells reset.
// No float op is in this file.
#include <algorithm>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kCrbSlice = DML_COALESCE_ELEMS_SLICE;  // dwords of a row that one item holds
constexpr int kCrbWaves = kCoBlock / 64;
constexpr int kCrbVec = kCrbSlice / 4 / 64;           // 16-byte vectors of a slice per lane
constexpr int64_t kCrbMaxBlocks = (int64_t)1 << 22;
static_assert(kCrbVec * 256 == kCrbSlice && kCrbWaves * kCrbSlice * 4 <= 65536 &&
                  kCrbRuns == DML_COMPACT_ROWS_BATCH_MAX_RUNS && kCrbRuns == 64,
              "a lane holds whole vectors of its slice; a block's slices fit LDS; a lane is a run");

// The run that holds row g of the runs laid end to end: the last q of [0, n) with off[q] <= g.
__device__ inline uint32_t crb_run(const PushCompactBatchP& a, uint32_t g, uint32_t n) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
// Closed before the call: only the call's last kernel writes these two, so all its kernels agree.
__device__ inline bool crb_shut(const ElemSink& k) { return (k.fver->idx != kNoPos) | (*k.neg != kNoPos); }

__global__ __launch_bounds__(kCoBlock) void k_crb_check(const PushCompactBatchP a) {
    if (crb_shut(a.sink)) return;  // a shut call touches no cell
    const uint32_t total = a.off[a.runs];
    for (int64_t g = (int64_t)blockIdx.x * kCoBlock + threadIdx.x; g < total; g += (int64_t)gridDim.x * kCoBlock) {
        const uint32_t q = crb_run(a, (uint32_t)g, (uint32_t)a.runs);
        const unsigned long long u = (uint32_t)g - a.off[q];
        const int64_t* keys = a.run[q].keys;
        const int32_t* ptr = a.run[q].ptr;
        const int32_t p0 = ptr[u], p1 = ptr[u + 1];
        const int64_t key = keys[u];
        const bool pf = p1 < p0 || (u == 0 && p0 != 0);
        const bool kf = u > 0 && key <= keys[u - 1];
        if (kf | pf) atomicMin(a.cells + kCrbForm + q, 2ull * u + (kf ? 0ull : 1ull));
        if (key < a.sink.first) atomicMin(a.cells + kCrbBad + q, 2ull * u);
        else if (key > a.sink.last) atomicMin(a.cells + kCrbBad + q, 2ull * u + 1ull);
    }
}

__global__ __launch_bounds__(64) void k_crb_stop(const PushCompactBatchP a) {
    const uint32_t q = threadIdx.x;
    unsigned long long word = 0ull;  // shut: nothing walks
    if (!crb_shut(a.sink)) {
        const bool in = q < (uint32_t)a.runs;
        const unsigned long long form = in ? a.cells[kCrbForm + q] : kNoPos;
        const unsigned long long bad = in ? a.cells[kCrbBad + q] : kNoPos;
        const unsigned long long faulty = __ballot((form != kNoPos) | (bad != kNoPos));
        word = (unsigned long long)a.runs;
        if (faulty != 0ull) {
            const uint32_t st = (uint32_t)__builtin_ctzll(faulty);
            // malformed, or an ascending run whose first key lies below the shard: nothing of it applies
            const unsigned long long none = __ballot((form != kNoPos) | (bad == 0ull));
            word = (unsigned long long)(st + (((none >> st) & 1ull) ? 0u : 1u)) | ((unsigned long long)(st + 1) << 8);
        }
    }
    if (q == 0) a.cells[kCrbStop] = word;
}

template <bool UNDO>
__global__ __launch_bounds__(kCoBlock) void k_crb_apply(const PushCompactBatchP a) {
    __shared__ u32x4 lds[kCrbWaves][kCrbSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* sl = (uint32_t*)lds[wave];
    const uint32_t nwalk = (uint32_t)(a.cells[kCrbStop] & 0xFFull);
    if (nwalk == 0) return;
    const unsigned long long rows = (unsigned long long)(a.sink.last - a.sink.first) + 1ull;
    const unsigned long long plane = rows * (unsigned long long)a.ncols;
    uint32_t frun = 0;  // UNDO: the failing run and element
    Undo f{0, 0};
    if constexpr (UNDO) {
        const unsigned long long ord = a.cells[kCrbOrd];
        if (ord == kNoPos) return;
        const unsigned long long cell = ord % plane;
        frun = (uint32_t)(ord / plane);
        f.row = (int64_t)(cell / (unsigned long long)a.ncols);
        f.col = (uint32_t)(cell % (unsigned long long)a.ncols);
    }
    const int64_t nitem = (int64_t)a.off[nwalk] * a.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kCrbWaves + wave; item < nitem; item += (int64_t)gridDim.x * kCrbWaves) {
        const uint32_t g = (uint32_t)(a.nslice == 1 ? item : item / a.nslice);
        const uint32_t c0 = (uint32_t)(item - (int64_t)g * a.nslice) * kCrbSlice;
        const uint32_t w = (uint32_t)a.ncols - c0 < (uint32_t)kCrbSlice ? (uint32_t)a.ncols - c0 : (uint32_t)kCrbSlice;
        const uint32_t r = crb_run(a, g, nwalk);
        const uint32_t i = g - a.off[r];
        const int64_t key = a.run[r].keys[i];
        if (key < a.sink.first || key > a.sink.last) continue;  // k_crb_check reported it; never an address
        // Lane q: where run q lists the key, if it does.
        uint32_t pos = i;
        bool hit = lane == r;
        if (lane < nwalk && lane != r) {
            const int64_t* kq = a.run[lane].keys;
            const uint32_t mq = a.off[lane + 1] - a.off[lane];
            uint32_t lo = 0, hi = mq;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (kq[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            pos = lo;
            hit = lo < mq && kq[lo] == key;
        }
        unsigned long long listed = __ballot(hit);
        if ((listed & ((1ull << r) - 1ull)) != 0ull) continue;  // the lowest run that lists the key owns its row
        const int32_t row = (int32_t)(key - a.sink.first);      // rows <= INT32_MAX
        int64_t keep = -1;
        if constexpr (UNDO) {
            listed &= ~((1ull << frun) - 1ull);  // runs in front of the failing one stay
            keep = undo_keep(f, row, c0, w);
            if (keep >= (int64_t)w - 1) listed &= ~(1ull << frun);
            if (listed == 0ull) continue;
        }
        uint8_t* p = (uint8_t*)a.sink.data + ((int64_t)row * a.ncols + c0) * 4;
        u32x4 sh[kCrbVec];   // the shard slice, in flight over the first walk
        u32x4 acc[kCrbVec];  // apply: .x ORs the updates (a vector no run changed is not stored); UNDO: what is taken back
#pragma unroll
        for (int k = 0; k < kCrbVec; ++k) {
            const uint32_t v = lane + 64 * k;
            sh[k] = acc[k] = u32x4{0u, 0u, 0u, 0u};
            if (4 * v < w) sh[k] = load_vec(p, v, w);
        }
        while (listed != 0ull) {
            const uint32_t q = (uint32_t)__builtin_ctzll(listed);
            listed &= listed - 1ull;
            const uint32_t u = (uint32_t)__shfl((int)pos, (int)q);
            const int32_t* ecol = a.run[q].ecol;
            const int32_t* eval = a.run[q].eval;
            const uint32_t s = (uint32_t)a.run[q].ptr[u], e = (uint32_t)a.run[q].ptr[u + 1];
            uint32_t ec = 0, ev = 0;
            if (s + lane < e) {
                ec = (uint32_t)ecol[s + lane];
                ev = (uint32_t)eval[s + lane];
            }
            zero_slice(sl, w, lane, 64);
            wave_phase();
            for (uint32_t b = s; b < e; b += 64) {
                const uint32_t pn = b + 64 + lane;
                uint32_t cn = 0, vn = 0;
                if (pn < e) {  // in flight over this batch's atomics
                    cn = (uint32_t)ecol[pn];
                    vn = (uint32_t)eval[pn];
                }
                if (b + lane < e) add_elem(sl, ec, ev, c0, w);
                ec = cn;
                ev = vn;
            }
            wave_phase();
            uint32_t low = kPeNone;
#pragma unroll
            for (int k = 0; k < kCrbVec; ++k) {
                const uint32_t v = lane + 64 * k;
                if (4 * v >= w) continue;
                u32x4 up = ((const u32x4*)sl)[v];
                if constexpr (UNDO) {
                    if (q == frun) {
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            if ((int64_t)(4 * v + d) <= keep) up[d] = 0u;
                    }
                    acc[k] += up;
                } else {
                    sh[k] += up;
                    acc[k].x |= up.x | up.y | up.z | up.w;
#pragma unroll
                    for (int d = 3; d >= 0; --d)
                        if (4 * v + d < w && (int32_t)sh[k][d] < 0) low = min(low, 4 * v + d);
                }
            }
            if constexpr (!UNDO) {
                if (__ballot(low != kPeNone) != 0ull) {  // rare: the wave's lowest failing column of this run
                    low = wave_min(low);
                    if (lane == 0)
                        atomicMin(a.cells + kCrbOrd,
                                  ((unsigned long long)q * rows + (unsigned long long)row) * (unsigned long long)a.ncols + c0 + low);
                }
            }
            wave_phase();  // the next run's zeroing comes after this read-back
        }
#pragma unroll
        for (int k = 0; k < kCrbVec; ++k) {
            const uint32_t v = lane + 64 * k;
            if constexpr (UNDO) {
                uint32_t none = kPeNone;
                update_vec<true>(p, v, w, sh[k], acc[k], -1, none);
            } else {
                if (4 * v < w && acc[k].x != 0u) store_vec(p, v, w, sh[k]);
            }
        }
    }
}

// Behind the call's kernels. A negative counter lies in a run that applied, so at or in front of
// stop: the reference never reaches stop's fault then. The call's cells reset.
__global__ __launch_bounds__(64) void k_crb_verdict(const PushCompactBatchP a) {
    const ElemSink& k = a.sink;
    const uint32_t q = threadIdx.x;
    if (q == 0 && !crb_shut(k)) {
        const unsigned long long ord = a.cells[kCrbOrd], stop = a.cells[kCrbStop] >> 8;
        if (ord != kNoPos) {
            const unsigned long long rows = (unsigned long long)(k.last - k.first) + 1ull;
            *k.neg = ord % (rows * (unsigned long long)a.ncols);
        } else if (stop != 0ull) {
            const unsigned long long form = a.cells[kCrbForm + stop - 1], bad = a.cells[kCrbBad + stop - 1];
            const int64_t* keys = a.run[stop - 1].keys;
            if (form != kNoPos) {
                k.fver->key = (form & 1ull) ? -1 : keys[form >> 1];
                k.fver->idx = kVerdictMalformed;
            } else {
                k.fver->key = keys[bad >> 1];
                k.fver->idx = bad >> 1;
            }
        }
    }
    __syncthreads();
    a.cells[kCrbForm + q] = kNoPos;
    a.cells[kCrbBad + q] = kNoPos;
    if (q == 0) a.cells[kCrbStop] = a.cells[kCrbOrd] = kNoPos;
}

}  // namespace

hipError_t launch_push_compact_batch(const PushCompactBatchP& a, hipStream_t st) {
    const int64_t total = a.off[a.runs], nitem = total * a.nslice;
    const int64_t cblocks = std::min<int64_t>((total + kCoBlock - 1) / kCoBlock, 1024);
    const int64_t blocks = std::min<int64_t>((nitem + kCrbWaves - 1) / kCrbWaves, kCrbMaxBlocks);
    hipLaunchKernelGGL(k_crb_check, dim3((unsigned)cblocks), dim3(kCoBlock), 0, st, a);
    hipLaunchKernelGGL(k_crb_stop, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL((k_crb_apply<false>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
    hipLaunchKernelGGL((k_crb_apply<true>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
    hipLaunchKernelGGL(k_crb_verdict, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace dml

// dml_coalesce_elems.hip — the coalescer's sum of ELEMENT updates (dml_coalesce_elems_device;
// DESIGN.md §4.14). A LightLDA worker moves a token of word w from topic `old` to topic `new`
// and pushes, per distinct word, the dense int32 row new - old (LightLDA.scala:224-239). On
// the device it holds the moves themselves: per occurrence (token) a key and per_occ
// (column, delta) pairs. These kernels turn them into the dense row per distinct key, as a
// plane or straight into push records, without a one-hot row per token ever existing.
//
// int32 adds wrap and commute, so the row of a key is exactly defined whatever the order
// of its adds: it accumulates in LDS with LDS integer atomics and no ordering machinery.
// Both kernels are output-stationary. An item is (distinct key u, slice of kElSlice dwords
// of its row); a row of more columns is several items, each walking the segment again and
// dropping the elements outside its slice. An element whose column is outside [0, cols)
// falls in no slice: it adds nothing and touches no memory.
//
//   k_co_elems       segments under lmin occurrences. One wave per item, kCoBlock / 64 waves
//                    per block, each with a private LDS slice. The wave zeroes the slice
//                    (16-byte LDS writes), walks the segment 64 occurrences at a time (lane
//                    l: index seg + l, its per_occ pairs by 8-byte loads, one ds_add_u32
//                    without return per element inside the slice; the next batch's indices
//                    are loaded before this batch's atomics), then reads the slice back as
//                    16-byte vectors and stores it with non-temporal 16-byte stores, 1 KiB
//                    per wave instruction, at the 4-byte-aligned addresses rows and record
//                    values have. A wave's LDS operations complete in issue order, so the
//                    three phases need no block barrier, no global atomic and no spin.
//   k_co_elems_long  segments of lmin and more (k_co_long_list's list, dml_coalesce_long.hip):
//                    one block of kElLongThreads threads per item, all its waves striding
//                    the segment into one shared slice; a barrier after the zeroing and one
//                    before the write-out, which is the same.
//
// LDS: k_co_elems 4 x 4 KiB = 16 KiB per block of 4 waves, so the 160 KiB of a CU hold 10
// blocks and the wave limit (32 per CU) binds first: 8 blocks, full occupancy.
// k_co_elems_long 4 KiB per block of 16 waves: two blocks per CU.
// No float op is in this file.
#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kElSlice = DML_COALESCE_ELEMS_SLICE;  // dwords of a row that one item sums
constexpr int kElWaves = kCoBlock / 64;
constexpr int kElLongThreads = 1024;
constexpr int64_t kElMaxBlocks = (int64_t)1 << 22;
constexpr int kElLongMaxBlocks = 2048;
static_assert(kElSlice % 256 == 0 && kElSlice >= 1000 && kElWaves * kElSlice * 4 <= 65536,
              "a slice is whole 1-KiB runs, holds config 5's row, and a block's slices fit LDS");

// The slice's w dwords to columns [c0, c0 + w) of row / record u, by threads t of nt: whole
// vectors as 16-byte stores, a ragged last vector's dwords singly. REC: the thread that
// stores column 0 stores the key in front of it.
template <bool REC>
__device__ inline void write_slice(const uint32_t* sl, const ElemsP& a, int64_t u, uint32_t c0, uint32_t w,
                                   int64_t key, uint32_t t, uint32_t nt) {
    uint8_t* o;
    if constexpr (REC) {
        uint8_t* r = a.out + u * a.rec.stride;
        if (t == 0 && c0 == 0) put_key(r, key, a.rec.kdw);
        o = r + 4 * a.rec.kdw + 4 * (int64_t)c0;
    } else {
        o = a.out + u * a.rowbytes + 4 * (int64_t)c0;
    }
    for (uint32_t v = t; 4 * v < w; v += nt) {
        const u32x4 x = ((const u32x4*)sl)[v];
        if (4 * v + 4 <= w) {
            stg16_nt(o + 16 * v, x);
        } else {
            const uint32_t q[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (uint32_t d = 0; d < 3; ++d)
                if (4 * v + d < w) stg32_nt(o + 16 * v + 4 * d, q[d]);
        }
    }
}

template <bool REC>
__global__ __launch_bounds__(kCoBlock) void k_co_elems(const ElemsP a) {
    __shared__ u32x4 lds[kElWaves][kElSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* sl = (uint32_t*)lds[threadIdx.x >> 6];
    const int64_t nitem = a.m * a.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kElWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kElWaves) {
        const int64_t u = a.nslice == 1 ? item : item / a.nslice;
        const uint32_t c0 = (uint32_t)(item - u * a.nslice) * kElSlice;
        const uint32_t w = (uint32_t)a.ncols - c0 < (uint32_t)kElSlice ? (uint32_t)a.ncols - c0 : (uint32_t)kElSlice;
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        if (e - s >= a.lmin) continue;  // the long route's: no walk and no store
        int64_t key = 0;
        if constexpr (REC) {
            if (lane == 0 && c0 == 0) key = a.rec.ukeys[u];  // in flight over the walk
        }
        uint32_t j = s + lane < e ? a.idx[s + lane] : 0u;
        zero_slice(sl, w, lane, 64);
        wave_phase();
        for (uint32_t base = s; base < e; base += 64) {
            const uint32_t pn = base + 64 + lane;
            const uint32_t jn = pn < e ? a.idx[pn] : 0u;  // in flight over this batch's atomics
            if (base + lane < e) add_occ(sl, a, j, c0, w);
            j = jn;
        }
        wave_phase();
        write_slice<REC>(sl, a, u, c0, w, key, lane, 64);
        wave_phase();  // the next item's zeroing comes after this read-back
    }
}

template <bool REC>
__global__ __launch_bounds__(kElLongThreads) void k_co_elems_long(const ElemsP a) {
    __shared__ u32x4 lds[kElSlice / 4];
    const uint32_t t = threadIdx.x;
    uint32_t* sl = (uint32_t*)lds;
    const int64_t nitem = (int64_t)a.route[0] * a.nslice;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t u = a.list[item / a.nslice];
        const uint32_t c0 = (uint32_t)(item % a.nslice) * kElSlice;
        const uint32_t w = (uint32_t)a.ncols - c0 < (uint32_t)kElSlice ? (uint32_t)a.ncols - c0 : (uint32_t)kElSlice;
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        int64_t key = 0;
        if constexpr (REC) {
            if (t == 0 && c0 == 0) key = a.rec.ukeys[u];  // in flight over the segment
        }
        uint32_t j = s + t < e ? a.idx[s + t] : 0u;
        zero_slice(sl, w, t, kElLongThreads);
        __syncthreads();
        for (uint32_t base = s; base < e; base += kElLongThreads) {
            const uint32_t pn = base + kElLongThreads + t;
            const uint32_t jn = pn < e ? a.idx[pn] : 0u;
            if (base + t < e) add_occ(sl, a, j, c0, w);
            j = jn;
        }
        __syncthreads();
        write_slice<REC>(sl, a, u, c0, w, key, t, kElLongThreads);
        __syncthreads();  // the next item's zeroing comes after every thread's read-back
    }
}

template <bool REC>
void launch_elems(const ElemsP& a, bool has_long, hipStream_t st) {
    if (has_long) {  // the list, then the long sums; the short route skips what they take
        co_launch_long_list(a.seg, a.n, a.m, a.lmin, a.list, a.route, st);
        const int64_t most = a.n / a.lmin;  // the list's capacity bounds the grid; the blocks read the count
        const unsigned grid = (unsigned)std::min<int64_t>(most * a.nslice, kElLongMaxBlocks);
        hipLaunchKernelGGL((k_co_elems_long<REC>), dim3(grid), dim3(kElLongThreads), 0, st, a);
    }
    const int64_t nitem = a.m * a.nslice;
    const int64_t blocks = std::min<int64_t>((nitem + kElWaves - 1) / kElWaves, kElMaxBlocks);
    hipLaunchKernelGGL((k_co_elems<REC>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
}

}  // namespace

int64_t co_elems_slices(int32_t ncols) { return ((int64_t)ncols + kElSlice - 1) / kElSlice; }

void co_launch_elems(const ElemsP& a, bool rec, bool has_long, hipStream_t st) {
    if (rec) launch_elems<true>(a, has_long, st);
    else launch_elems<false>(a, has_long, st);
}

}  // namespace dml

// dml_coalesce_long.hip — the coalescer's sum of LONG segments: the keys
// with lmin occurrences and more, which the walks of dml_coalesce.hip leave out. The adds of
// one output element are the same chain in the same order as there, +0.0 first and one
// add_ref per occurrence; what changes is who fetches: a whole block, many rows at a time.
//
//   k_co_long_list        u in [0, m): a segment of >= lmin occurrences appends u to the list
//                         (one atomic on the count word, so the list's order is arbitrary; no
//                         output byte depends on it) and adds its length to the second word
//   k_co_sum_long         rows of 16 bytes and more. An item is (long key, kLongSlice-byte
//                         column slice of its row); one block owns it for the whole segment.
//                         All kLongThreads threads fetch a tile of kLongTile consecutive
//                         occurrences' slices with 16-byte non-temporal loads into registers
//                         and store it to LDS as [occurrence][slice]; thread t then adds
//                         element t of the slice down the tile, in occurrence order, into
//                         one register. While a tile is added the next tile's rows and the
//                         indices of the one after are in flight (two LDS buffers, one
//                         barrier per tile).
//   k_co_sum_long_narrow  rows under 16 bytes: one wave per long key; kLongNarrowBatch x 64
//                         occurrences are gathered one per lane and added in lane order by
//                         a readlane loop while the next ones load
//
// add_chunk: kLongChunk adds without add_ref's NaN fix-up, which is exact unless the chunk
// ends NaN (a NaN never leaves an accumulator); only then is the chunk redone from its saved
// start with add_ref. The element's chain is then one add per occurrence.
//
// REC (dml_coalesce_pack_device): both sum kernels' owner stores go into push record u
// (RecP, dml_coalesce_dev.h) instead of row u of a dense plane; nothing else differs.
#include <type_traits>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kLongThreads = 512;
constexpr int kLongTile = DML_COALESCE_LONG_TILE;    // occurrences of a tile
constexpr int kLongSlice = DML_COALESCE_LONG_SLICE;  // bytes of a row that one block sums
constexpr int kLongVecRow = kLongSlice / 16;         // 16-byte vectors of a slice
constexpr int kLongRowStep = kLongThreads / kLongVecRow;             // rows between a thread's vectors
constexpr int kLongVec = kLongTile * kLongVecRow / kLongThreads;     // vectors a thread loads per tile
constexpr int kLongChunk = 8;        // adds between two NaN checks
constexpr int kLongNarrowBatch = 4;  // x 64 occurrences per step of the narrow kernel
constexpr int kLongMaxBlocks = 2048;
static_assert(kLongSlice % 16 == 0 && kLongThreads % kLongVecRow == 0 && kLongVec * kLongThreads == kLongTile * kLongVecRow &&
                  kLongSlice / 4 <= kLongThreads && 2 * kLongTile * kLongSlice <= 65536 && kCoSpanBytes % kLongSlice == 0,
              "a tile is a whole number of vectors per thread, two tiles fit LDS");

__global__ __launch_bounds__(kCoBlock) void k_co_long_list(const uint32_t* __restrict__ seg, int64_t n, int64_t m,
                                                           uint32_t lmin, uint32_t* __restrict__ list,
                                                           uint32_t* __restrict__ route) {
    const int64_t u = (int64_t)blockIdx.x * kCoBlock + threadIdx.x;
    if (u >= m) return;
    const uint32_t s = seg[u], e = u + 1 < m ? seg[u + 1] : (uint32_t)n;
    if (e - s < lmin) return;
    list[atomicAdd(&route[0], 1u)] = (uint32_t)u;  // at most n / lmin segments are this long
    atomicAdd(&route[1], e - s);
}

// ((a + x[0]) + x[1]) + ... as kLongChunk add_ref would give it, bit for bit.
template <typename T>
__device__ inline T add_chunk(T a, const T (&x)[kLongChunk]) {
    T p = a;
#pragma unroll
    for (int d = 0; d < kLongChunk; ++d) p = Elem<T>::add(p, x[d]);
    if constexpr (!std::is_same<T, int32_t>::value) {
        if (p != p) {  // a NaN came in or was created: the chunk again, with the reference's NaN
            p = a;
#pragma unroll
            for (int d = 0; d < kLongChunk; ++d) p = add_ref(p, x[d]);
        }
    }
    return p;
}

template <typename T, bool REC>
__global__ __launch_bounds__(kLongThreads) void k_co_sum_long(const LongP a, int64_t nslice) {
    __shared__ u32x4 lds[2][kLongTile * kLongVecRow];
    const int t = threadIdx.x;
    const int r0 = t / kLongVecRow, vb = (t % kLongVecRow) * 16;  // this thread's first row and its vector's byte
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const int64_t nitem = (int64_t)a.route[0] * nslice;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t u = a.list[item / nslice];
        const int64_t soff = (item % nslice) * kLongSlice;
        const int w = (int)(a.rowbytes - soff < kLongSlice ? a.rowbytes - soff : kLongSlice);  // bytes of this slice
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        int64_t key = 0;
        if constexpr (REC) {
            if (t == 0 && soff == 0) key = a.rec.ukeys[u];  // in flight over the segment
        }
        const bool col = vb < w;
        // the slice's last vector, when it is no whole one, is loaded shifted back to end at the
        // slice's last byte (the row is >= 16 bytes, so the load stays inside the row) and only
        // its trailing dwords go to LDS
        const bool ragged = col && vb + 16 > w;
        const int first = ragged ? 4 - ((w - vb) >> 2) : 0;
        const uint8_t* src = a.values + soff + (ragged ? w - 16 : vb);
        const int nel = w / (int)sizeof(T);
        uint32_t j[kLongVec];
        u32x4 x[kLongVec];

        // x: this thread's vectors of the tile at sorted position `b`, by the indices in j;
        // then j: its indices of the tile after that one
        auto fetch = [&](uint32_t b) {
#pragma unroll
            for (int i = 0; i < kLongVec; ++i) {
                x[i] = zero;
                if (col && b + r0 + i * kLongRowStep < e) x[i] = ldg16_nt(src + (int64_t)j[i] * a.rowbytes);
            }
#pragma unroll
            for (int i = 0; i < kLongVec; ++i) {
                const uint32_t p = b + kLongTile + r0 + i * kLongRowStep;
                j[i] = (col && p < e) ? a.idx[p] : 0u;
            }
        };
        auto stage = [&](uint32_t b, u32x4* buf) {
#pragma unroll
            for (int i = 0; i < kLongVec; ++i) {
                const int r = r0 + i * kLongRowStep;
                if (!col || b + r >= e) continue;
                if (!ragged) {
                    buf[r * kLongVecRow + (vb >> 4)] = x[i];
                } else {
                    uint32_t* d = (uint32_t*)buf + r * (kLongSlice / 4) + (vb >> 2);
                    const uint32_t q[4] = {x[i].x, x[i].y, x[i].z, x[i].w};
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        if (k >= first) d[k - first] = q[k];
                }
            }
        };

#pragma unroll
        for (int i = 0; i < kLongVec; ++i) {
            const uint32_t p = s + r0 + i * kLongRowStep;
            j[i] = (col && p < e) ? a.idx[p] : 0u;
        }
        fetch(s);
        stage(s, lds[0]);
        __syncthreads();
        T acc = T(0);
        int cur = 0;
        for (uint32_t b = s; b < e; b += kLongTile, cur ^= 1) {
            const bool more = e - b > (uint32_t)kLongTile;
            if (more) fetch(b + kLongTile);
            if (t < nel) {
                const int cnt = more ? kLongTile : (int)(e - b);
                const T* row = (const T*)lds[cur] + t;
                constexpr int stride = kLongSlice / (int)sizeof(T);
                int r = 0;
                for (; r + kLongChunk <= cnt; r += kLongChunk) {
                    T xs[kLongChunk];
#pragma unroll
                    for (int d = 0; d < kLongChunk; ++d) xs[d] = row[(r + d) * stride];
                    acc = add_chunk<T>(acc, xs);
                }
                for (; r < cnt; ++r) acc = add_ref(acc, row[r * stride]);
            }
            if (more) stage(b + kLongTile, lds[cur ^ 1]);
            __syncthreads();
        }
        if (t < nel) {
            uint8_t* o;
            if constexpr (REC) {  // the owner of the row's first element writes the key in front of it
                uint8_t* r = a.out + u * a.rec.stride;
                if (t == 0 && soff == 0) put_key(r, key, a.rec.kdw);
                o = r + 4 * a.rec.kdw + soff + (int64_t)t * sizeof(T);
            } else {
                o = a.out + u * a.rowbytes + soff + (int64_t)t * sizeof(T);
            }
            if constexpr (sizeof(T) == 4) {
                stg32_nt(o, __builtin_bit_cast(uint32_t, acc));
            } else {
                const uint64_t q = __builtin_bit_cast(uint64_t, acc);
                stg32_nt(o, (uint32_t)q);
                stg32_nt(o + 4, (uint32_t)(q >> 32));
            }
        }
    }
}

// Element c of the row lane `l` holds in x, as every lane's (uniform) value.
template <typename T>
__device__ inline T lane_elem(const u32x4& x, int c, int l) {
    if constexpr (sizeof(T) == 4) {
        return Elem<T>::from_bits((uint32_t)__builtin_amdgcn_readlane((int)x[c], l), 0u);
    } else {
        return Elem<T>::from_bits((uint32_t)__builtin_amdgcn_readlane((int)x.x, l),
                                  (uint32_t)__builtin_amdgcn_readlane((int)x.y, l));
    }
}

// Rows of RDW = 1, 2 or 3 dwords. A slot past the segment's end holds +0.0, which leaves an
// accumulator that started at +0.0 as it is (k_co_sum's argument).
template <typename T, int RDW, bool REC>
__global__ __launch_bounds__(kCoBlock) void k_co_sum_long_narrow(const LongP a) {
    constexpr int E = RDW * 4 / (int)sizeof(T);  // elements of a row
    constexpr int NB = kLongNarrowBatch;
    constexpr uint32_t kStep = 64 * NB;
    const uint32_t lane = threadIdx.x & 63;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const uint32_t nlong = a.route[0];
    for (uint32_t li = blockIdx.x * (kCoBlock / 64) + (threadIdx.x >> 6); li < nlong; li += gridDim.x * (kCoBlock / 64)) {
        const int64_t u = a.list[li];
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        int64_t key = 0;
        if constexpr (REC) {
            if (lane == 0) key = a.rec.ukeys[u];  // in flight over the segment
        }
        uint32_t j[NB];
        u32x4 x[NB], y[NB];
        // y: the rows of the step at sorted position `b`, by j; then j: the indices of the step after it
        auto fetch = [&](uint32_t b) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                y[k] = zero;
                if (b + k * 64 + lane < e) y[k] = load_narrow<RDW>(a.values + (int64_t)j[k] * (RDW * 4));
            }
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const uint32_t p = b + kStep + k * 64 + lane;
                j[k] = p < e ? a.idx[p] : 0u;
            }
        };
#pragma unroll
        for (int k = 0; k < NB; ++k) j[k] = s + k * 64 + lane < e ? a.idx[s + k * 64 + lane] : 0u;
        fetch(s);
        T acc[E];
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = T(0);
        for (uint32_t b = s; b < e; b += kStep) {
#pragma unroll
            for (int k = 0; k < NB; ++k) x[k] = y[k];
            if (e - b > kStep) fetch(b + kStep);
#pragma unroll
            for (int k = 0; k < NB; ++k) {
#pragma unroll 1
                for (int l0 = 0; l0 < 64 && b + k * 64 + l0 < e; l0 += kLongChunk) {
#pragma unroll
                    for (int c = 0; c < E; ++c) {
                        T xs[kLongChunk];
#pragma unroll
                        for (int d = 0; d < kLongChunk; ++d) xs[d] = lane_elem<T>(x[k], c, l0 + d);
                        acc[c] = add_chunk<T>(acc[c], xs);
                    }
                }
            }
        }
        if (lane == 0) {
            uint8_t* o;
            if constexpr (REC) {  // key, row, pad: the record's dwords in ascending order
                uint8_t* r = a.out + u * a.rec.stride;
                put_key(r, key, a.rec.kdw);
                o = r + 4 * a.rec.kdw;
            } else {
                o = a.out + u * (RDW * 4);
            }
#pragma unroll
            for (int c = 0; c < E; ++c) {
                if constexpr (sizeof(T) == 4) {
                    stg32_nt(o + 4 * c, __builtin_bit_cast(uint32_t, acc[c]));
                } else {
                    const uint64_t q = __builtin_bit_cast(uint64_t, acc[c]);
                    stg32_nt(o, (uint32_t)q);
                    stg32_nt(o + 4, (uint32_t)(q >> 32));
                }
            }
            if constexpr (REC) {
                if (a.rec.pad) stg32_nt(o + RDW * 4, 0u);
            }
        }
    }
}

template <typename T, bool REC>
void launch_long(const LongP& a, hipStream_t st) {
    const int64_t most = a.n / a.lmin;  // the list's capacity bounds the grid; the blocks read the count
    if (a.rowbytes >= 16) {
        const int64_t nslice = (a.rowbytes + kLongSlice - 1) / kLongSlice;
        const unsigned grid = (unsigned)std::min<int64_t>(most * nslice, kLongMaxBlocks);
        hipLaunchKernelGGL((k_co_sum_long<T, REC>), dim3(grid), dim3(kLongThreads), 0, st, a, nslice);
        return;
    }
    const dim3 grid((unsigned)std::min<int64_t>((most + kCoBlock / 64 - 1) / (kCoBlock / 64), kLongMaxBlocks)), blk(kCoBlock);
    if constexpr (sizeof(T) == 8) {
        hipLaunchKernelGGL((k_co_sum_long_narrow<T, 2, REC>), grid, blk, 0, st, a);
    } else {
        switch ((int)(a.rowbytes / 4)) {
            case 1: hipLaunchKernelGGL((k_co_sum_long_narrow<T, 1, REC>), grid, blk, 0, st, a); break;
            case 2: hipLaunchKernelGGL((k_co_sum_long_narrow<T, 2, REC>), grid, blk, 0, st, a); break;
            default: hipLaunchKernelGGL((k_co_sum_long_narrow<T, 3, REC>), grid, blk, 0, st, a); break;
        }
    }
}

template <bool REC>
void launch_long_of(const LongP& a, int32_t value_type, hipStream_t st) {
    if (value_type == DML_ELEMENT_TYPE_FLOAT) launch_long<float, REC>(a, st);
    else if (value_type == DML_ELEMENT_TYPE_DOUBLE) launch_long<double, REC>(a, st);
    else launch_long<int32_t, REC>(a, st);
}

}  // namespace

void co_launch_long_list(const uint32_t* seg, int64_t n, int64_t m, uint32_t lmin, uint32_t* list, uint32_t* route,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_co_long_list, dim3((unsigned)((m + kCoBlock - 1) / kCoBlock)), dim3(kCoBlock), 0, st, seg, n, m,
                       lmin, list, route);
}

void co_launch_long(const LongP& a, int32_t value_type, bool rec, hipStream_t st) {
    co_launch_long_list(a.seg, a.n, a.m, a.lmin, a.list, a.route, st);
    if (rec) launch_long_of<true>(a, value_type, st);
    else launch_long_of<false>(a, value_type, st);
}

}  // namespace dml

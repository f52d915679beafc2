// dml_fetch_planes.hip — the plane fetch of dml_store_fetch_planes_device.
//
// A worker on the store's own GPU wants a T[n][cols] plane indexed by occurrence (and
// AdaGrad's alpha plane beside it), not handleFetch's record stream. These kernels go shard ->
// planes in one pass: the occurrence keys as they are, repeats and any order included, no sort,
// no records, nothing staged. Bytes pass through as dwords: no float instruction touches them.
//
//   k_fetch_planes<DUAL, D>   row-stationary, the shape of k_co_sum (dml_coalesce.hip): a group
//                 of G lanes owns one plane row, or one 1-KiB span of a longer row, one 16-byte
//                 vector per lane; G is the smallest power of two >= the span's vectors. A wave
//                 carries 64 / G neighbouring occurrences, so one store instruction writes one
//                 contiguous run of the plane. The group's first lane loads the key, checks it
//                 once and the row index is broadcast inside the group (ds_bpermute): no LDS
//                 array, no barrier. A wave keeps D such slots in flight: D keys, then D (DUAL:
//                 2 D) 16-byte shard loads, then the non-temporal stores. DUAL: the same lane,
//                 holding the same row offset, moves the alpha array's vector to the alpha plane
//                 (the AdaGrad store holds data and alpha as two arrays: nothing is interleaved).
//                 A row's last vector, when the row is no multiple of 16 bytes, is loaded shifted
//                 back so that it ends at the row's last byte (rows here are >= 16 bytes) and only
//                 its trailing dwords are stored: k_co_sum's rule.
//   k_fetch_planes_narrow<RDW, DUAL, U>   rows of 1, 2 or 3 dwords (the array stores, 1-3 f32 /
//                 i32 columns, one f64): one lane per occurrence, U occurrences per thread a
//                 block apart, so the key loads and the plane stores are coalesced across the wave.
//
// A key outside [first, last] (compared as 64-bit values) is never turned into an address: its
// group issues no load and no store, and the lane that loaded it reports the list index by
// atomicMin on `bad` (k_fetch_verdict, dml_fetch.hip, takes it from there). That atomic decides
// no output byte. Repeated keys re-read their row through L2: the shard loads are cached ones.
#include <algorithm>

#include "dml_fetch_line.h"

namespace dml {

namespace {

constexpr int kPlBlock = 256;
constexpr int64_t kPlSpanBytes = 1024;  // 64 lanes x 16 bytes
constexpr int64_t kPlMaxBlocks = (int64_t)1 << 22;
// The shipped slots per wave / occurrences per thread, by measurement: two, and
// one with both planes (a DUAL slot is two vector loads already).
constexpr int kPlDepth = 2, kPlDepthDual = 1;

struct PlanesP {
    const uint8_t* data;   // the shard's rows
    const uint8_t* alpha;  // DUAL: AdaGrad's alpha array, rows of the same rowbytes
    const int64_t* keys;   // int64[n]
    uint8_t* values;       // T[n][cols], 4-byte aligned
    uint8_t* aplane;       // DUAL: float[n][cols], 4-byte aligned
    int64_t n, first, last;
    int64_t rowbytes;      // >= 16
    int64_t nspan;         // 1-KiB spans of a row
    int64_t ntask;         // wave tasks of one span: ceil(n / (D x 64 / G))
    int32_t lgG;           // log2 of the lanes of a group
    unsigned long long* bad;
};

__device__ inline void stg8_nt(void* p, u32x2 v) { __builtin_nontemporal_store(v, (DML_GLOBAL u32x2_u*)p); }

// The trailing `keep` dwords (1 .. 3) of a vector that was loaded shifted back to end at the
// row's last byte, or the whole vector (keep == 4), to `o`.
__device__ inline void put_vec(uint8_t* o, const u32x4& x, int keep) {
    if (keep == 4) {
        stg16_nt(o, x);
        return;
    }
    const int first = 4 - keep;
    const uint32_t q[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int d = 1; d < 4; ++d)
        if (d >= first) stg32_nt(o + 4 * (d - first), q[d]);
}

template <bool DUAL, int D>
__global__ __launch_bounds__(kPlBlock) void k_fetch_planes(const PlanesP a) {
    const int lane = threadIdx.x & 63;
    const int G = 1 << a.lgG, gl = lane & (G - 1), per = 64 >> a.lgG;
    const int64_t step = (int64_t)per * D;
    // the spans of a long row are blockIdx.y's (one span: the loop runs once)
    for (int64_t span = blockIdx.y; span < a.nspan; span += gridDim.y) {
        const int64_t vb = (span * 64 + gl) * 16;  // this lane's vector, as a byte of the row
        const int64_t left = a.rowbytes - vb;
        // dwords this lane stores: 4, a ragged row's last 1 .. 3, or 0 past the row's end (G rounds up)
        const int keep = left >= 16 ? 4 : left > 0 ? (int)(left >> 2) : 0;
        const int64_t off = left >= 16 ? vb : a.rowbytes - 16;  // the last vector ends at the row's last byte
        for (int64_t w = (int64_t)blockIdx.x * (kPlBlock / 64) + (threadIdx.x >> 6); w < a.ntask;
             w += (int64_t)gridDim.x * (kPlBlock / 64)) {
            const int64_t j0 = w * step + (lane >> a.lgG);
            int64_t key[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {  // D keys in flight, one load per group
                const int64_t j = j0 + d * per;
                key[d] = 0;
                if (gl == 0 && j < a.n) key[d] = a.keys[j];
            }
            int32_t mine[D];  // the group's first lane: the row of its key; -1 refused, or past the list
            unsigned long long refused = kNoPos;  // the lowest list index this lane refused
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int64_t j = j0 + d * per;
                const bool own = gl == 0 && j < a.n, good = key[d] >= a.first && key[d] <= a.last;
                mine[d] = own && good ? (int32_t)(key[d] - a.first) : -1;  // rows <= INT32_MAX
                if (own && !good && refused == kNoPos) refused = (unsigned long long)j;
            }
            if (refused != kNoPos && span == 0) atomicMin(a.bad, refused);
            u32x4 x[D], y[D];
            bool act[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {  // every load before the first store
                const int32_t row = __shfl(mine[d], 0, G);
                act[d] = row >= 0 && keep != 0;
                if (act[d]) {  // x[d], y[d] of an idle lane stay unset: they are never stored
                    const int64_t src = (int64_t)row * a.rowbytes + off;
                    x[d] = ldg16(a.data + src);
                    if (DUAL) y[d] = ldg16(a.alpha + src);
                }
            }
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (!act[d]) continue;
                const int64_t dst = (j0 + d * per) * a.rowbytes + vb;
                put_vec(a.values + dst, x[d], keep);
                if (DUAL) put_vec(a.aplane + dst, y[d], keep);
            }
        }
    }
}

template <int RDW>
__device__ inline u32x4 get_narrow(const uint8_t* p) {
    u32x4 x = {0u, 0u, 0u, 0u};
    if (RDW == 2) {
        const u32x2 t = ldg8((const uint32_t*)p);
        x.x = t.x; x.y = t.y;
    } else {
        x.x = ldg32(p);
        if (RDW == 3) { x.y = ldg32(p + 4); x.z = ldg32(p + 8); }
    }
    return x;
}
template <int RDW>
__device__ inline void put_narrow(uint8_t* o, const u32x4& x) {
    if (RDW == 2) {
        u32x2 t;
        t.x = x.x; t.y = x.y;
        stg8_nt(o, t);
    } else {
        stg32_nt(o, x.x);
        if (RDW == 3) { stg32_nt(o + 4, x.y); stg32_nt(o + 8, x.z); }
    }
}

template <int RDW, bool DUAL, int U>
__global__ __launch_bounds__(kPlBlock) void k_fetch_planes_narrow(const int64_t* __restrict__ keys, int64_t n,
                                                                  int64_t first, int64_t last,
                                                                  const uint8_t* __restrict__ data,
                                                                  const uint8_t* __restrict__ alpha,
                                                                  uint8_t* __restrict__ values,
                                                                  uint8_t* __restrict__ aplane,
                                                                  unsigned long long* __restrict__ bad) {
    constexpr int64_t kTile = (int64_t)kPlBlock * U;
    for (int64_t j0 = (int64_t)blockIdx.x * kTile + threadIdx.x; j0 < n; j0 += (int64_t)gridDim.x * kTile) {
        int64_t key[U], row[U];  // row -1: refused, or past the list
#pragma unroll
        for (int u = 0; u < U; ++u) {  // U coalesced key loads in flight
            const int64_t j = j0 + u * kPlBlock;
            key[u] = 0;
            if (j < n) key[u] = keys[j];
        }
        unsigned long long refused = kNoPos;  // the lowest list index this lane refused
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t j = j0 + u * kPlBlock;
            const bool good = key[u] >= first && key[u] <= last;
            row[u] = j < n && good ? key[u] - first : -1;
            if (j < n && !good && refused == kNoPos) refused = (unsigned long long)j;
        }
        if (refused != kNoPos) atomicMin(bad, refused);
        u32x4 x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (row[u] < 0) continue;
            x[u] = get_narrow<RDW>(data + row[u] * (RDW * 4));
            if (DUAL) y[u] = get_narrow<RDW>(alpha + row[u] * (RDW * 4));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (row[u] < 0) continue;
            const int64_t dst = (j0 + u * kPlBlock) * (RDW * 4);
            put_narrow<RDW>(values + dst, x[u]);
            if (DUAL) put_narrow<RDW>(aplane + dst, y[u]);
        }
    }
}

template <bool DUAL, int D>
void launch_wide(PlanesP a, hipStream_t st) {
    const int64_t step = (int64_t)(64 >> a.lgG) * D;
    a.ntask = (a.n + step - 1) / step;
    const int64_t blocks = std::min<int64_t>((a.ntask + kPlBlock / 64 - 1) / (kPlBlock / 64), kPlMaxBlocks);
    const int64_t spans = std::min<int64_t>(a.nspan, 65535);
    hipLaunchKernelGGL((k_fetch_planes<DUAL, D>), dim3((unsigned)blocks, (unsigned)spans), dim3(kPlBlock), 0, st, a);
}

template <int RDW, bool DUAL, int U>
void launch_narrow(const PlanesP& a, hipStream_t st) {
    const int64_t tile = (int64_t)kPlBlock * U;
    const int64_t blocks = std::min<int64_t>((a.n + tile - 1) / tile, kPlMaxBlocks);
    hipLaunchKernelGGL((k_fetch_planes_narrow<RDW, DUAL, U>), dim3((unsigned)blocks), dim3(kPlBlock), 0, st, a.keys, a.n,
                       a.first, a.last, a.data, a.alpha, a.values, a.aplane, a.bad);
}

template <bool DUAL, int D>
void launch_d(const PlanesP& a, hipStream_t st) {
    if (a.rowbytes >= 16) return launch_wide<DUAL, D>(a, st);
    switch ((int)(a.rowbytes / 4)) {
        case 1: return launch_narrow<1, DUAL, D>(a, st);
        case 2: return launch_narrow<2, DUAL, D>(a, st);
        default: return launch_narrow<3, DUAL, D>(a, st);
    }
}

template <bool DUAL>
void launch_dual(const PlanesP& a, int depth, hipStream_t st) {
    switch (depth ? depth : DUAL ? kPlDepthDual : kPlDepth) {
        case 1: return launch_d<DUAL, 1>(a, st);
        case 2: return launch_d<DUAL, 2>(a, st);
        default: return launch_d<DUAL, 4>(a, st);  // 8 slots: the wide kernel's flags spill SGPRs
    }
}

}  // namespace

hipError_t launch_fetch_planes(const void* shard, const float* alpha, int64_t rowbytes, const int64_t* keys, int64_t n,
                               int64_t first, int64_t last, void* values, void* alpha_plane, unsigned long long* bad,
                               int depth, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    PlanesP a;
    a.data = (const uint8_t*)shard;
    a.alpha = (const uint8_t*)alpha;
    a.keys = keys;
    a.values = (uint8_t*)values;
    a.aplane = (uint8_t*)alpha_plane;
    a.n = n;
    a.first = first;
    a.last = last;
    a.rowbytes = rowbytes;
    a.nspan = (rowbytes + kPlSpanBytes - 1) / kPlSpanBytes;
    const int64_t vecs = (std::min(rowbytes, kPlSpanBytes) + 15) / 16;
    a.ntask = 0;
    a.lgG = 0;
    while ((1 << a.lgG) < vecs) ++a.lgG;
    a.bad = bad;
    if (alpha_plane) launch_dual<true>(a, depth, st);
    else launch_dual<false>(a, depth, st);
    return hipGetLastError();
}

}  // namespace dml

// dml_push_planes.hip — the plane push of dml_store_push_planes_device: the
// coalescer's ordered sums with a store's shard as their sink.
//
// A worker on the store's own GPU holds a gradient plane T[n][cols] indexed by occurrence. The
// record route writes the m summed rows as push records, and the store's reduce reads them back
// and indexes their keys a second time. Here the order stage and k_co_heads (dml_coalesce.hip)
// run as they are, and the sum kernels below end in the store's own per-element update of the
// shard row instead of a store of the sum: per distinct key, ascending, element i of the update
// row is ((+0.0 + v[j1][i]) + v[j2][i]) + ... over the key's occurrences in list order
// (add_ref), and then row[i] = row[i] + u (AdaGrad: delta += u x u, alpha where delta ends
// above 1, the strict rise of delta the element's maxDelta candidate). No sum is ever in HBM.
//
//   k_pp_walk<T, ADA>     the shape of k_co_sum: a group of G lanes owns one distinct key's row,
//                 or one 1-KiB span of it, one 16-byte vector per lane. The group's first lane
//                 loads the key, checks it once and broadcasts the shard row (-1: refused). The
//                 lane's shard vector (ADA: and its delta vector) is loaded before the walk and
//                 is in flight over it; the walk is k_co_sum's (kPpBatch indices per group,
//                 kPpDepth rows' loads ahead of the adds); then the update and the stores. A
//                 ragged row's last vector is loaded shifted back, values and shard alike; its
//                 leading elements repeat the previous lane's and are neither stored nor
//                 candidates.
//   k_pp_narrow<T, RDW, ADA>   rows of 1-3 dwords (arrays, 1-3 f32 columns, one f64): one lane
//                 per distinct key.
//   k_pp_long<T, ADA>, k_pp_long_narrow<T, RDW, ADA>   keys with lmin occurrences and more, which
//                 the two above leave out: k_co_sum_long's staging (a block per kPpSlice bytes
//                 of the row, kPpTile occurrences at a time through LDS, two buffers) and
//                 k_co_sum_long_narrow's readlane chain, the same adds in the same order. The
//                 shard slice is loaded before the first tile.
//
// A key outside [first, last] (64-bit compare) is never turned into an address: its group loads
// no value and no shard byte and stores nothing; the lowest such distinct-key index goes to
// `bad` by atomicMin, which decides no output byte. The keys ascend, so ukeys[0] < first means
// the record route would stop at its first record: every kernel then returns before any store.
// AdaGrad: one candidate per block, positions are shard element indices (ascending keys are
// ascending row-major order), finalised once per call by k_maxdelta_elems (dml_moments.hip).
#include <algorithm>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kPpBatch = DML_COALESCE_BATCH, kPpDepth = DML_COALESCE_DEPTH;
constexpr int kPpThreads = 512;                      // the long kernel's block
constexpr int kPpTile = DML_COALESCE_LONG_TILE;      // occurrences of a tile
constexpr int kPpSlice = DML_COALESCE_LONG_SLICE;    // bytes of a row that one block sums
constexpr int kPpVecRow = kPpSlice / 16;             // 16-byte vectors of a slice
constexpr int kPpRowStep = kPpThreads / kPpVecRow;   // rows between a thread's vectors
constexpr int kPpVec = kPpTile * kPpVecRow / kPpThreads;  // vectors a thread loads per tile
constexpr int kPpChunk = 8;        // adds between two NaN checks (add_chunk)
constexpr int kPpNarrowBatch = 4;  // x 64 occurrences per step of the long narrow kernel
constexpr int64_t kPpMaxBlocks = (int64_t)1 << 22;
constexpr int kPpLongMaxBlocks = 2048;
static_assert(kPpBatch % kPpDepth == 0 && kPpSlice % 16 == 0 && kPpThreads % kPpVecRow == 0 &&
                  kPpVec * kPpThreads == kPpTile * kPpVecRow && kPpSlice / 4 <= kPpThreads &&
                  2 * kPpTile * kPpSlice <= 65536 && kCoSpanBytes % kPpSlice == 0 && kPushCands <= kMomentBlocks,
              "the coalescer's tile sizes; the candidates fit the store's buffer");

__device__ inline void stg32(void* p, uint32_t v) { *(DML_GLOBAL uint32_t*)p = v; }

// A thread's running maxDelta candidate.
struct Cand {
    bool ok = false;
    float v = 0.f;
    uint64_t p = kNoPos;
};

// Nothing of the call is applied: an earlier call's verdict is closed and unreported, or the
// list's smallest key lies below the shard. Block-uniform.
__device__ inline bool pp_shut(const PushP& a) { return (a.sink.verdict->idx != kNoPos) | (a.ukeys[0] < a.sink.first); }
// ... and the second case's report, by one thread of the kernel every call launches.
__device__ inline void pp_report_low(const PushP& a) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.sink.verdict->idx == kNoPos && a.ukeys[0] < a.sink.first)
        atomicMin(a.sink.bad, 0ull);
}
// The shard row of distinct key u, -1 refused (reported when `report`).
__device__ inline int32_t pp_row(const PushP& a, int64_t u, bool report) {
    const int64_t key = a.ukeys[u];
    if (key >= a.sink.first && key <= a.sink.last) return (int32_t)(key - a.sink.first);  // rows <= INT32_MAX
    if (report) atomicMin(a.sink.bad, (unsigned long long)u);
    return -1;
}

// The store's update of one element of a row the call lists once (FloatMatrixStore.java:200-222;
// FloatMatrixStoreAdaGrad.java:262-277): x = x + u as every reduce adds it (Elem<T>::add). ADA:
// d += u x u, a strict rise is the element's maxDelta candidate at shard element `ei`, and where
// d ends above 1 the new alpha is left in na (returns true).
template <typename T, bool ADA>
__device__ __forceinline__ bool push_elem(const PushSink& k, T& x, T u, float& d, float& na, uint64_t ei, Cand& c) {
    x = Elem<T>::add(x, u);
    if constexpr (ADA) {
        const float nd = __fadd_rn(d, __fmul_rn(u, u));
        if (nd > d && cand_better(true, nd, ei, c.ok, c.v, c.p)) {
            c.ok = true;
            c.v = nd;
            c.p = ei;
        }
        d = nd;
        if (nd > 1.0f) {
            na = ada_alpha(nd, k.initial_alpha, k.factor, k.min_alpha);
            return true;
        }
    }
    return false;
}

// The update of one vector of a row, at byte `eoff` of the shard: sh (ADA: dl) is what the shard
// (delta) holds there, acc the sums. The first `lead` dwords repeat the previous lane's elements
// (a ragged row's last vector, shifted back): they are not updated, stored or candidates. Only the
// first `ndw` dwords exist (narrow rows; 4 otherwise).
template <typename T, bool ADA>
__device__ inline void apply_vec(const PushSink& k, int64_t eoff, int lead, int ndw, u32x4 sh, u32x4 dl, u32x4 acc,
                                 Cand& c) {
    constexpr int VEC = Elem<T>::VEC, EDW = (int)sizeof(T) / 4;
    T x[VEC], u[VEC];
    float d[4] = {0.f, 0.f, 0.f, 0.f}, na[4] = {0.f, 0.f, 0.f, 0.f};
    bool big[4] = {false, false, false, false};
    unpack<T>(sh, x);
    unpack<T>(acc, u);
    if constexpr (ADA) unpack<float>(dl, d);
    bool all_big = lead == 0 && ndw == 4;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if (e * EDW < lead || e * EDW >= ndw) continue;
        big[e] = push_elem<T, ADA>(k, x[e], u[e], d[e], na[e], (uint64_t)(eoff >> 2) + e, c);
        all_big = all_big && big[e];
    }
    const u32x4 xs = pack<T>(x);
    uint8_t* o = k.data + eoff;
    if (lead == 0 && ndw == 4) {
        stg16(o, xs);
        if constexpr (ADA) stg16((uint8_t*)k.delta + eoff, pack<float>(d));
    } else {
        const uint32_t q[4] = {xs.x, xs.y, xs.z, xs.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < lead || w >= ndw) continue;
            stg32(o + 4 * w, q[w]);
            if constexpr (ADA) stg32((uint8_t*)k.delta + eoff + 4 * w, __float_as_uint(d[w]));
        }
    }
    if constexpr (ADA) {
        if (all_big) {
            stg16((uint8_t*)k.alpha + eoff, pack<float>(na));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (big[e]) stg32((uint8_t*)k.alpha + eoff + 4 * e, __float_as_uint(na[e]));
        }
    }
}

// The block's candidate, one per block of an ADA launch (every thread of the block calls it).
template <int WPB>
__device__ inline void put_cand(const PushP& a, Cand& c) {
    cand_block_best<WPB>(c.ok, c.v, c.p);
    if (threadIdx.x == 0) a.cand[blockIdx.x] = cand_of(c.ok, c.v, c.p);
}

template <typename T, bool ADA>
__global__ __launch_bounds__(kCoBlock) void k_pp_walk(const PushP a) {
    const int lane = threadIdx.x & 63;
    const int G = 1 << a.lgG, gl = lane & (G - 1), per = 64 >> a.lgG;
    const int B = G < kPpBatch ? G : kPpBatch;
    const int64_t nitem = a.m * a.nspan;
    const int64_t nwave = pp_shut(a) ? 0 : (nitem + per - 1) / per;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    Cand c;
    pp_report_low(a);
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
        // dwords in front of a ragged row's last vector that repeat the previous lane's
        const int lead = act && vb + 16 > a.rowbytes ? 4 - (int)((a.rowbytes - vb) >> 2) : 0;
        // a lane past the row's end (G rounds up) walks the last vector too: one address, one request
        const int64_t off = vb + 16 > a.rowbytes ? a.rowbytes - 16 : vb;
        uint32_t s = 0, e = 0;
        if (live) {
            s = a.seg[u];
            e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        }
        const bool lng = e - s >= a.lmin;  // the long kernel's: no key check, no walk and no store here
        int32_t mine = -1;
        if (live && !lng && gl == 0) mine = pp_row(a, u, span == 0);
        const int32_t row = __shfl(mine, 0, G);
        if (row < 0) e = s;
        const bool on = act && row >= 0;
        const int64_t eoff = (int64_t)row * a.rowbytes + off;
        u32x4 sh = zero, dl = zero;
        if (on) {  // in flight over the walk
            sh = ldg16(a.sink.data + eoff);
            if constexpr (ADA) dl = ldg16((const uint8_t*)a.sink.delta + eoff);
        }
        u32x4 acc = zero;
        for (uint32_t base = s; base < e; base += (uint32_t)B) {
            const int cnt = e - base < (uint32_t)B ? (int)(e - base) : B;
            const uint32_t own = gl < cnt ? a.idx[base + gl] : 0u;
            int k0 = 0;
            for (; k0 + kPpDepth <= cnt; k0 += kPpDepth) {  // whole steps: every load is unconditional
                u32x4 x[kPpDepth];
#pragma unroll
                for (int d = 0; d < kPpDepth; ++d) {
                    const uint32_t j = (uint32_t)__shfl((int)own, (k0 + d) & (G - 1), G);
                    x[d] = ldg16_nt(a.values + (int64_t)j * a.rowbytes + off);
                }
#pragma unroll
                for (int d = 0; d < kPpDepth; ++d) acc = add_vec<T>(acc, x[d]);
            }
            if (k0 < cnt) {  // the batch's last 1 .. kPpDepth - 1 rows; +0.0 leaves the sums as they are
                u32x4 x[kPpDepth - 1];
#pragma unroll
                for (int d = 0; d < kPpDepth - 1; ++d) {
                    const uint32_t j = (uint32_t)__shfl((int)own, (k0 + d) & (G - 1), G);
                    x[d] = zero;
                    if (k0 + d < cnt) x[d] = ldg16_nt(a.values + (int64_t)j * a.rowbytes + off);
                }
#pragma unroll
                for (int d = 0; d < kPpDepth - 1; ++d) acc = add_vec<T>(acc, x[d]);
            }
        }
        if (on) apply_vec<T, ADA>(a.sink, eoff, lead, 4, sh, dl, acc, c);
    }
    if constexpr (ADA) put_cand<kCoBlock / 64>(a, c);
}

// The shard's (cached) counterpart of load_narrow.
template <int RDW>
__device__ inline u32x4 shard_narrow(const uint8_t* p) {
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

template <typename T, int RDW, bool ADA>
__global__ __launch_bounds__(kCoBlock) void k_pp_narrow(const PushP a) {
    const int64_t m = pp_shut(a) ? 0 : a.m;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    Cand c;
    pp_report_low(a);
    for (int64_t u = (int64_t)blockIdx.x * kCoBlock + threadIdx.x; u < m; u += (int64_t)gridDim.x * kCoBlock) {
        const uint32_t s = a.seg[u], e = u + 1 < m ? a.seg[u + 1] : (uint32_t)a.n;
        if (e - s >= a.lmin) continue;  // the long kernel's
        const int32_t row = pp_row(a, u, true);
        if (row < 0) continue;
        const int64_t eoff = (int64_t)row * (RDW * 4);
        const u32x4 sh = shard_narrow<RDW>(a.sink.data + eoff);  // in flight over the walk
        u32x4 dl = zero;
        if constexpr (ADA) dl = shard_narrow<RDW>((const uint8_t*)a.sink.delta + eoff);
        u32x4 acc = zero;
        uint32_t k0 = s;
        for (; k0 + kPpDepth <= e; k0 += kPpDepth) {  // whole steps
            uint32_t j[kPpDepth];
            u32x4 x[kPpDepth];
#pragma unroll
            for (int d = 0; d < kPpDepth; ++d) j[d] = a.idx[k0 + d];
#pragma unroll
            for (int d = 0; d < kPpDepth; ++d) x[d] = load_narrow<RDW>(a.values + (int64_t)j[d] * (RDW * 4));
#pragma unroll
            for (int d = 0; d < kPpDepth; ++d) acc = add_vec<T>(acc, x[d]);
        }
        for (; k0 < e; ++k0)  // the last 1 .. kPpDepth - 1 occurrences
            acc = add_vec<T>(acc, load_narrow<RDW>(a.values + (int64_t)a.idx[k0] * (RDW * 4)));
        apply_vec<T, ADA>(a.sink, eoff, 0, RDW, sh, dl, acc, c);
    }
    if constexpr (ADA) put_cand<kCoBlock / 64>(a, c);
}

// ((a + x[0]) + x[1]) + ... as kPpChunk add_ref would give it, bit for bit (dml_coalesce_long.hip's
// add_chunk: exact unless the chunk ends NaN; only then is it redone with add_ref).
template <typename T>
__device__ inline T add_chunk(T a, const T (&x)[kPpChunk]) {
    T p = a;
#pragma unroll
    for (int d = 0; d < kPpChunk; ++d) p = Elem<T>::add(p, x[d]);
    if (p != p) {
        p = a;
#pragma unroll
        for (int d = 0; d < kPpChunk; ++d) p = add_ref(p, x[d]);
    }
    return p;
}

// One element of the shard, and its store: dwords, the row is 4-byte aligned only.
template <typename T>
__device__ inline void put_elem(uint8_t* p, T v) {
    if constexpr (sizeof(T) == 4) {
        stg32(p, __builtin_bit_cast(uint32_t, v));
    } else {
        const uint64_t q = __builtin_bit_cast(uint64_t, v);
        stg32(p, (uint32_t)q);
        stg32(p + 4, (uint32_t)(q >> 32));
    }
}

template <typename T, bool ADA>
__global__ __launch_bounds__(kPpThreads) void k_pp_long(const PushP a, int64_t nslice) {
    __shared__ u32x4 lds[2][kPpTile * kPpVecRow];
    const int t = threadIdx.x;
    const int r0 = t / kPpVecRow, vb = (t % kPpVecRow) * 16;  // this thread's first row and its vector's byte
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const int64_t nitem = pp_shut(a) ? 0 : (int64_t)a.route[0] * nslice;
    Cand c;
    for (int64_t item = blockIdx.x; item < nitem; item += gridDim.x) {
        const int64_t u = a.list[item / nslice];
        const int64_t soff = (item % nslice) * kPpSlice;
        const int32_t row = pp_row(a, u, t == 0 && soff == 0);  // block-uniform
        if (row < 0) continue;
        const int w = (int)(a.rowbytes - soff < kPpSlice ? a.rowbytes - soff : kPpSlice);  // bytes of this slice
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        const int nel = w / (int)sizeof(T);
        // this thread's element of the shard slice, in flight over the segment
        const int64_t eoff = (int64_t)row * a.rowbytes + soff + (int64_t)t * sizeof(T);
        T x = T(0);
        float d = 0.f, na = 0.f;
        if (t < nel) {
            x = Elem<T>::load(a.sink.data + eoff);
            if constexpr (ADA) d = __uint_as_float(ldg32((const uint8_t*)a.sink.delta + eoff));
        }
        const bool col = vb < w;
        // the slice's last vector, when it is no whole one, is loaded shifted back to end at the
        // slice's last byte (the row is >= 16 bytes) and only its trailing dwords go to LDS
        const bool ragged = col && vb + 16 > w;
        const int first = ragged ? 4 - ((w - vb) >> 2) : 0;
        const uint8_t* src = a.values + soff + (ragged ? w - 16 : vb);
        uint32_t j[kPpVec];
        u32x4 v[kPpVec];

        // v: this thread's vectors of the tile at sorted position `b`, by the indices in j;
        // then j: its indices of the tile after that one
        auto fetch = [&](uint32_t b) {
#pragma unroll
            for (int i = 0; i < kPpVec; ++i) {
                v[i] = zero;
                if (col && b + r0 + i * kPpRowStep < e) v[i] = ldg16_nt(src + (int64_t)j[i] * a.rowbytes);
            }
#pragma unroll
            for (int i = 0; i < kPpVec; ++i) {
                const uint32_t p = b + kPpTile + r0 + i * kPpRowStep;
                j[i] = (col && p < e) ? a.idx[p] : 0u;
            }
        };
        auto stage = [&](uint32_t b, u32x4* buf) {
#pragma unroll
            for (int i = 0; i < kPpVec; ++i) {
                const int r = r0 + i * kPpRowStep;
                if (!col || b + r >= e) continue;
                if (!ragged) {
                    buf[r * kPpVecRow + (vb >> 4)] = v[i];
                } else {
                    uint32_t* dst = (uint32_t*)buf + r * (kPpSlice / 4) + (vb >> 2);
                    const uint32_t q[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                    for (int k = 1; k < 4; ++k)
                        if (k >= first) dst[k - first] = q[k];
                }
            }
        };

#pragma unroll
        for (int i = 0; i < kPpVec; ++i) {
            const uint32_t p = s + r0 + i * kPpRowStep;
            j[i] = (col && p < e) ? a.idx[p] : 0u;
        }
        fetch(s);
        stage(s, lds[0]);
        __syncthreads();
        T acc = T(0);
        int cur = 0;
        for (uint32_t b = s; b < e; b += kPpTile, cur ^= 1) {
            const bool more = e - b > (uint32_t)kPpTile;
            if (more) fetch(b + kPpTile);
            if (t < nel) {
                const int cnt = more ? kPpTile : (int)(e - b);
                const T* rowp = (const T*)lds[cur] + t;
                constexpr int stride = kPpSlice / (int)sizeof(T);
                int r = 0;
                for (; r + kPpChunk <= cnt; r += kPpChunk) {
                    T xs[kPpChunk];
#pragma unroll
                    for (int q = 0; q < kPpChunk; ++q) xs[q] = rowp[(r + q) * stride];
                    acc = add_chunk<T>(acc, xs);
                }
                for (; r < cnt; ++r) acc = add_ref(acc, rowp[r * stride]);
            }
            if (more) stage(b + kPpTile, lds[cur ^ 1]);
            __syncthreads();
        }
        if (t < nel) {
            const bool big = push_elem<T, ADA>(a.sink, x, acc, d, na, (uint64_t)(eoff >> 2), c);
            put_elem<T>(a.sink.data + eoff, x);
            if constexpr (ADA) {
                stg32((uint8_t*)a.sink.delta + eoff, __float_as_uint(d));
                if (big) stg32((uint8_t*)a.sink.alpha + eoff, __float_as_uint(na));
            }
        }
    }
    if constexpr (ADA) put_cand<kPpThreads / 64>(a, c);
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

// Rows of RDW = 1, 2 or 3 dwords: one wave per long key, k_co_sum_long_narrow's chain; lane 0
// holds the shard row over the segment and applies the update.
template <typename T, int RDW, bool ADA>
__global__ __launch_bounds__(kCoBlock) void k_pp_long_narrow(const PushP a) {
    constexpr int E = RDW * 4 / (int)sizeof(T);  // elements of a row
    constexpr int NB = kPpNarrowBatch;
    constexpr uint32_t kStep = 64 * NB;
    const uint32_t lane = threadIdx.x & 63;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const uint32_t nlong = pp_shut(a) ? 0u : a.route[0];
    Cand c;
    for (uint32_t li = blockIdx.x * (kCoBlock / 64) + (threadIdx.x >> 6); li < nlong; li += gridDim.x * (kCoBlock / 64)) {
        const int64_t u = a.list[li];
        const int32_t row = pp_row(a, u, lane == 0);  // wave-uniform
        if (row < 0) continue;
        const uint32_t s = a.seg[u], e = u + 1 < a.m ? a.seg[u + 1] : (uint32_t)a.n;
        const int64_t eoff = (int64_t)row * (RDW * 4);
        u32x4 sh = zero, dl = zero;
        if (lane == 0) {  // in flight over the segment
            sh = shard_narrow<RDW>(a.sink.data + eoff);
            if constexpr (ADA) dl = shard_narrow<RDW>((const uint8_t*)a.sink.delta + eoff);
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
        for (int q = 0; q < E; ++q) acc[q] = T(0);
        for (uint32_t b = s; b < e; b += kStep) {
#pragma unroll
            for (int k = 0; k < NB; ++k) x[k] = y[k];
            if (e - b > kStep) fetch(b + kStep);
#pragma unroll
            for (int k = 0; k < NB; ++k) {
#pragma unroll 1
                for (int l0 = 0; l0 < 64 && b + k * 64 + l0 < e; l0 += kPpChunk) {
#pragma unroll
                    for (int q = 0; q < E; ++q) {
                        T xs[kPpChunk];
#pragma unroll
                        for (int d = 0; d < kPpChunk; ++d) xs[d] = lane_elem<T>(x[k], q, l0 + d);
                        acc[q] = add_chunk<T>(acc[q], xs);
                    }
                }
            }
        }
        if (lane == 0) {
            T full[Elem<T>::VEC] = {};
#pragma unroll
            for (int q = 0; q < E; ++q) full[q] = acc[q];
            apply_vec<T, ADA>(a.sink, eoff, 0, RDW, sh, dl, pack<T>(full), c);
        }
    }
    if constexpr (ADA) put_cand<kCoBlock / 64>(a, c);
}

template <typename T, bool ADA>
void launch_long(const PushP& a, hipStream_t st) {
    const int64_t most = a.n / a.lmin;  // the list's capacity bounds the grid; the blocks read the count
    const int64_t cap = ADA ? kPushLongCands : kPpLongMaxBlocks;
    if (a.rowbytes >= 16) {
        const int64_t nslice = (a.rowbytes + kPpSlice - 1) / kPpSlice;
        const unsigned grid = (unsigned)std::min<int64_t>(ADA ? cap : most * nslice, cap);
        hipLaunchKernelGGL((k_pp_long<T, ADA>), dim3(grid), dim3(kPpThreads), 0, st, a, nslice);
        return;
    }
    // ADA: every block of the grid the finalize counts on writes its candidate
    const dim3 grid((unsigned)std::min<int64_t>(ADA ? cap : (most + kCoBlock / 64 - 1) / (kCoBlock / 64), cap)), blk(kCoBlock);
    if constexpr (sizeof(T) == 8) {
        hipLaunchKernelGGL((k_pp_long_narrow<T, 2, ADA>), grid, blk, 0, st, a);
    } else {
        switch ((int)(a.rowbytes / 4)) {
            case 1: hipLaunchKernelGGL((k_pp_long_narrow<T, 1, ADA>), grid, blk, 0, st, a); break;
            case 2: hipLaunchKernelGGL((k_pp_long_narrow<T, 2, ADA>), grid, blk, 0, st, a); break;
            default: hipLaunchKernelGGL((k_pp_long_narrow<T, 3, ADA>), grid, blk, 0, st, a); break;
        }
    }
}

// Returns the blocks launched (ADA: the candidates written).
template <typename T, bool ADA>
int64_t launch_walk(const PushP& a, hipStream_t st) {
    const int64_t cap = ADA ? kPushWalkCands : kPpMaxBlocks;
    if (a.rowbytes < 16) {
        const int64_t blocks = std::min<int64_t>((a.m + kCoBlock - 1) / kCoBlock, cap);
        const dim3 grid((unsigned)blocks), blk(kCoBlock);
        if constexpr (sizeof(T) == 8) {
            hipLaunchKernelGGL((k_pp_narrow<T, 2, ADA>), grid, blk, 0, st, a);
        } else {
            switch ((int)(a.rowbytes / 4)) {
                case 1: hipLaunchKernelGGL((k_pp_narrow<T, 1, ADA>), grid, blk, 0, st, a); break;
                case 2: hipLaunchKernelGGL((k_pp_narrow<T, 2, ADA>), grid, blk, 0, st, a); break;
                default: hipLaunchKernelGGL((k_pp_narrow<T, 3, ADA>), grid, blk, 0, st, a); break;
            }
        }
        return blocks;
    }
    const int64_t per = 64 >> a.lgG, nwave = (a.m * a.nspan + per - 1) / per;
    const int64_t blocks = std::min<int64_t>((nwave + kCoBlock / 64 - 1) / (kCoBlock / 64), cap);
    hipLaunchKernelGGL((k_pp_walk<T, ADA>), dim3((unsigned)blocks), dim3(kCoBlock), 0, st, a);
    return blocks;
}

template <typename T, bool ADA>
hipError_t launch_t(const PushP& a, bool has_long, hipStream_t st) {
    PushP w = a, l = a;
    w.cand = a.sink.cand;
    const int64_t nw = launch_walk<T, ADA>(w, st);
    if (has_long) {
        co_launch_long_list(a.seg, a.n, a.m, a.lmin, const_cast<uint32_t*>(a.list), const_cast<uint32_t*>(a.route), st);
        l.cand = a.sink.cand + nw;
        launch_long<T, ADA>(l, st);
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if constexpr (ADA)
        return launch_maxdelta_elems(a.sink.cand, nw + (has_long ? kPushLongCands : 0), a.sink.md, a.sink.first,
                                     a.sink.cols, st);
    return hipSuccess;
}

}  // namespace

hipError_t launch_push_planes(const PushP& a, int32_t value_type, bool has_long, hipStream_t st) {
    if (a.sink.md) return launch_t<float, true>(a, has_long, st);
    if (value_type == DML_ELEMENT_TYPE_DOUBLE) return launch_t<double, false>(a, has_long, st);
    return launch_t<float, false>(a, has_long, st);
}

}  // namespace dml

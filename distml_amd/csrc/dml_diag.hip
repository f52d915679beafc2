// dml_diag.hip — kernels no product path calls: what dml_store_diag.hip's dml_synth_* and
// dml_diag_* entry points launch, for tests, scripts and the legs of the benchmark.
//
//   k_synth_dense, k_synth_sparse, k_synth_fill  synthetic pushes and shard contents
//                     (DESIGN.md §Synthetic data; CPU twin: oracle/dml_oracle.c)
//   k_stream          read / copy streaming ceilings
//   k_ring_rs         the local HBM footprint of one rank's ring reduce-scatter
//   k_rmw_floor, k_gather_floor, k_dense_floor  floors the sparse leaf, the int32 row
//                     reduce and the flat dense / AdaGrad reduces are judged against
//
// They mirror no reference code; the floors move the same bytes as the product kernel
// named at each. Driven by dml_store_diag.hip.
#include "dml_device.h"
#include "dml_launch.h"

#include <algorithm>

namespace dml {

// ---------------------------------------------------------------------------
// Synthetic data (DESIGN.md §Synthetic data; CPU twin: oracle/dml_oracle.c).
__device__ inline int32_t synth_grad_int(uint64_t h) {
    const int32_t s = (int32_t)(h & 0xFFFF) + (int32_t)((h >> 16) & 0xFFFF) + (int32_t)((h >> 32) & 0xFFFF) +
                      (int32_t)((h >> 48) & 0xFFFF);
    return s - 131070;
}
__device__ inline void put_value(uint8_t* p, int vtype, uint64_t h) {
    if (vtype == kF32) {
        st32(p, __float_as_uint((float)synth_grad_int(h) * 0x1p-25f));
    } else if (vtype == kF64) {
        const uint64_t u = __builtin_bit_cast(uint64_t, (double)synth_grad_int(h) * 0x1p-25);
        st32(p, (uint32_t)u); st32(p + 4, (uint32_t)(u >> 32));
    } else {
        st32(p, (uint32_t)((int32_t)(h % 5) - 2));
    }
}
__device__ inline void put_key(uint8_t* p, int K, int64_t key) {
    st32(p, (uint32_t)key);
    if (K == 8) st32(p + 4, (uint32_t)((uint64_t)key >> 32));
}

// perm: record r -> row (pa*r + pc) mod n; host guarantees pa < 2^32, r < 2^32.
__global__ void k_synth_dense(uint8_t* __restrict__ out, int K, int vtype, int64_t first, int64_t shard_rows,
                              int64_t nrec, int32_t cols, uint64_t s0, uint64_t pa, uint64_t pc) {
    const int V = vtype == kF64 ? 8 : 4;
    const int64_t stride = K + (int64_t)V * cols;
    const int64_t total = nrec * (int64_t)cols;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / cols;
        const int32_t c = (int32_t)(t - r * cols);
        const uint64_t row = ((pa * (uint64_t)r) % (uint64_t)shard_rows + pc) % (uint64_t)shard_rows;
        uint8_t* rec = out + r * stride;
        if (c == 0) put_key(rec, K, first + (int64_t)row);
        put_value(rec + K + (int64_t)V * c, vtype, splitmix64_dev(s0 + row * (uint64_t)cols + (uint64_t)c));
    }
}
hipError_t launch_synth_dense(uint8_t* out, int K, int vtype, int64_t first, int64_t shard_rows, int64_t nrec,
                              int32_t cols, uint64_t s0, uint64_t pa, uint64_t pc, hipStream_t st) {
    hipLaunchKernelGGL(k_synth_dense, dim3(8192), dim3(256), 0, st, out, K, vtype, first, shard_rows, nrec, cols, s0, pa, pc);
    return hipGetLastError();
}

__global__ void k_synth_sparse(uint8_t* __restrict__ out, int K, int vtype, int value_stride, int64_t first,
                               int64_t key_space, int64_t nrec, uint64_t s0, uint64_t pa, uint64_t pc) {
    const int64_t stride = K + value_stride;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t i = ((pa * (uint64_t)r) % (uint64_t)key_space + pc) % (uint64_t)key_space;
        uint8_t* rec = out + r * stride;
        put_key(rec, K, first + (int64_t)i);
        for (int z = 0; z < value_stride; z += 4) st32(rec + K + z, 0u);
        put_value(rec + K, vtype, splitmix64_dev(s0 + i));
    }
}
hipError_t launch_synth_sparse(uint8_t* out, int K, int vtype, int value_stride, int64_t first, int64_t key_space,
                               int64_t nrec, uint64_t s0, uint64_t pa, uint64_t pc, hipStream_t st) {
    hipLaunchKernelGGL(k_synth_sparse, dim3(8192), dim3(256), 0, st, out, K, vtype, value_stride, first, key_space, nrec,
                       s0, pa, pc);
    return hipGetLastError();
}

__global__ void k_synth_fill(int vtype, void* p, int64_t n, uint64_t s0) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = splitmix64_dev(s0 + (uint64_t)i);
        if (vtype == kF32) ((float*)p)[i] = (float)((int32_t)(h % 100) - 50) * 0x1p-17f;
        else if (vtype == kF64) ((double*)p)[i] = (double)((int32_t)(h % 100) - 50) * 0x1p-17;
        else ((int32_t*)p)[i] = 64 + (int32_t)(h % 51);
    }
}
hipError_t launch_synth_fill(int vtype, void* p, int64_t n, uint64_t s0, hipStream_t st) {
    hipLaunchKernelGGL(k_synth_fill, dim3(8192), dim3(256), 0, st, vtype, p, n, s0);
    return hipGetLastError();
}

// Streaming ceilings (diagnostic): 4 independent 16-B nt loads per lane in
// flight, contiguous 4 KiB per wave step. COPY writes what it reads; READ folds
// the loads into one word that is stored only if it hits a sentinel.
template <bool COPY>
__global__ __launch_bounds__(256) void k_stream(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                                int64_t n16) {
    const int64_t lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    uint32_t fold = 0;
    for (int64_t base = wave * 256; base < n16; base += nwaves * 256) {
        u32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = base + j * 64 + lane;
            v[j] = ldg16_nt(src + (i < n16 ? i : 0) * 16);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = base + j * 64 + lane;
            if constexpr (COPY) {
                if (i < n16) stg16(dst + i * 16, v[j]);
            } else {
                fold ^= v[j].x ^ v[j].y ^ v[j].z ^ v[j].w;
            }
        }
    }
    if constexpr (!COPY)
        if (fold == 0x9E3779B9u) *(uint32_t*)dst = fold;
}

// Ring reduce-scatter footprint (diagnostic, bench.py --emulate-rs): the local HBM
// traffic of one rank's ring reduce-scatter, as ONE kernel of `channels` blocks
// (RCCL runs one persistent block per channel). world - 1 steps: step s reads the
// chunk the rank sends, (rank - s - 1) mod world, plus the chunk that arrived at
// step s - 1, and writes their sum where the next rank's write would land (a local
// stand-in for the peer's write into this rank's buffer); the last step adds the
// rank's own chunk into recv. A thread owns the same vectors in every step, so the
// steps need no synchronization. Values are meaningless (no peer contributes).
template <typename T>
__global__ __launch_bounds__(256) void k_ring_rs(const T* __restrict__ part, T* __restrict__ recv,
                                                 T* __restrict__ land, int64_t chunk16, int world, int rank) {
    constexpr int VEC = Elem<T>::VEC, U = 8;  // 8 vectors per thread per step in flight, as RCCL's unrolled copies
    const uint8_t* P = (const uint8_t*)part;
    uint8_t* Lb[2] = {(uint8_t*)land, (uint8_t*)land + chunk16 * 16};
    const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < chunk16; i0 += nthr * U) {
        for (int s2 = 0; s2 < world; ++s2) {
            const int64_t c = s2 == world - 1 ? rank : ((rank - s2 - 1) % world + world) % world;
            u32x4 xa[U], ya[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * nthr;
                xa[u] = i < chunk16 ? ldg16_nt(P + (c * chunk16 + i) * 16) : u32x4{0u, 0u, 0u, 0u};
                ya[u] = (s2 > 0 && i < chunk16) ? ldg16_nt(Lb[s2 & 1] + i * 16) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + u * nthr;
                if (i >= chunk16) continue;
                T x[VEC], y[VEC];
                unpack<T>(xa[u], x);
                unpack<T>(ya[u], y);
#pragma unroll
                for (int e = 0; e < VEC; ++e) x[e] = Elem<T>::add(x[e], y[e]);
                stg16_nt((s2 == world - 1 ? (uint8_t*)recv : Lb[(s2 + 1) & 1]) + i * 16, pack<T>(x));
            }
        }
    }
}

hipError_t launch_ring_rs(int vtype, const void* part, void* recv, void* land, int64_t chunk_bytes, int world,
                          int rank, int channels, hipStream_t st) {
    const int64_t n16 = chunk_bytes / 16;
    if (n16 <= 0) return hipSuccess;
    const dim3 g((unsigned)std::max(1, channels)), blk(256);
    if (vtype == kF64)
        hipLaunchKernelGGL(k_ring_rs<double>, g, blk, 0, st, (const double*)part, (double*)recv, (double*)land, n16,
                           world, rank);
    else if (vtype == kI32)
        hipLaunchKernelGGL(k_ring_rs<int32_t>, g, blk, 0, st, (const int32_t*)part, (int32_t*)recv, (int32_t*)land,
                           n16, world, rank);
    else
        hipLaunchKernelGGL(k_ring_rs<float>, g, blk, 0, st, (const float*)part, (float*)recv, (float*)land, n16,
                           world, rank);
    return hipGetLastError();
}

// Random-RMW floor (diagnostic): one plain 4-B read-modify-write per update over a
// globally sorted index list — the best case of config 3's scatter-add (every update
// in address order, no partition), against which the leaf kernel is judged.
// Repeated indices race: the array's values are not meaningful afterwards.
__global__ __launch_bounds__(256) void k_rmw_floor(float* __restrict__ a, const uint32_t* __restrict__ idx,
                                                   const float* __restrict__ v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t k = idx[i];
        a[k] = a[k] + v[i];
    }
}

hipError_t launch_rmw_floor(float* a, const uint32_t* idx, const float* v, int64_t n, hipStream_t st, LaunchEv ev) {
    if (n <= 0) return hipSuccess;
    // one update per thread up to 2^28 updates (config 3: 32e6), grid-stride beyond
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)1 << 20);
    return launch_k(k_rmw_floor, dim3(grid), dim3(256), 0, st, ev, a, idx, v, n);
}

// Row-gather floor (diagnostic, config 5): the touched rows of an int32 shard in row
// order, each read once, every record that lists it (listed in push order by the
// caller, `addr` = the record's value bytes) gathered and added, the row written once
// — the same bytes as the IntMatrixStore reduce with no key index, slot table,
// negativity check or error bookkeeping. One wave per touched row (<= 256 16-B
// vectors: cols <= 1024), four records' loads in flight, XCD-contiguous blocks as the
// product's DEPTH-3 reduce. The values are meaningful (plain wrapping int adds).
__global__ __launch_bounds__(256) void k_gather_floor(int32_t* __restrict__ shard, int32_t cols,
                                                      const int32_t* __restrict__ trow, const int32_t* __restrict__ tptr,
                                                      const uint64_t* __restrict__ addr, int64_t ntouched) {
    const int64_t w = xcd_block() * 4 + (threadIdx.x >> 6);
    if (w >= ntouched) return;
    const int lane = threadIdx.x & 63, nvec = cols / 4;
    uint8_t* rowp = (uint8_t*)(shard + (int64_t)trow[w] * cols);
    const int32_t b0 = tptr[w], b1 = tptr[w + 1];
    u32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        acc[j] = v < nvec ? ldg16_nt(rowp + v * 16) : u32x4{0u, 0u, 0u, 0u};
    }
    for (int32_t e = b0; e < b1; e += 4) {
        u32x4 x[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t a = e + k < b1 ? uni64(addr[e + k]) : 0ull;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = lane + 64 * j;
                x[k][j] = (a && v < nvec) ? ldg16_nt((const uint8_t*)a + v * 16) : u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += x[k][j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        if (v < nvec) stg16_nt(rowp + v * 16, acc[j]);
    }
}

hipError_t launch_gather_floor(int32_t* shard, int32_t cols, const int32_t* trow, const int32_t* tptr,
                               const uint64_t* addr, int64_t ntouched, hipStream_t st, LaunchEv ev) {
    if (ntouched <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((ntouched + 3) / 4);
    return launch_k(k_gather_floor, dim3(grid), dim3(256), 0, st, ev, shard, cols, trow, tptr, addr, ntouched);
}

// Dense stream floor (diagnostic, config 4 and its AdaGrad variant): the shard's
// elements in order, each read once with the same element of every full-range push
// whose records are rows in order (record r = row r, values 4 bytes after the key),
// summed in push order and written once — to `out` (the speculative second buffer,
// as k_flat_ident writes it) or in place; ADA: delta += u·u beside it (AdaGrad's
// data / delta stream, k_ada_ident's bytes). No key checks, slot tables or maxDelta
// bookkeeping: the plain stream of the same bytes, over the same allocations.
template <bool ADA>
__global__ __launch_bounds__(256) void k_dense_floor(const float* __restrict__ data, float* __restrict__ out,
                                                     float* __restrict__ delta, Batch bt, int nb, int64_t stride,
                                                     int K, int32_t cols, int64_t nvec) {
    constexpr int U = 2, D = 4;
    const int64_t v0 = xcd_block() * (256 * U) + threadIdx.x;
    int64_t off[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * 256, e = v * 4;
        ok[u] = v < nvec;
        off[u] = (e / cols) * stride + K + (e % cols) * 4;
    }
    u32x4 acc[U], dl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * 256;
        acc[u] = ok[u] ? ldg16_nt((const uint8_t*)data + v * 16) : u32x4{0u, 0u, 0u, 0u};
        if (ADA) dl[u] = ok[u] ? ldg16_nt((const uint8_t*)delta + v * 16) : u32x4{0u, 0u, 0u, 0u};
    }
    for (int b = 0; b < nb; b += D) {
        u32x4 x[D][U];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int u = 0; u < U; ++u)
                x[d][u] = (b + d < nb && ok[u]) ? ldg16_nt(bt.base[b + d] + off[u]) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (b + d >= nb) break;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g = __uint_as_float(x[d][u][e]);
                    acc[u][e] = __float_as_uint(__fadd_rn(__uint_as_float(acc[u][e]), g));
                    if (ADA) dl[u][e] = __float_as_uint(__fadd_rn(__uint_as_float(dl[u][e]), __fmul_rn(g, g)));
                }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
        const int64_t v = v0 + u * 256;
        stg16_nt((uint8_t*)out + v * 16, acc[u]);
        if (ADA) stg16_nt((uint8_t*)delta + v * 16, dl[u]);
    }
}

hipError_t launch_dense_floor(const float* data, float* out, float* delta, const Batch& bt, int nb, int64_t stride,
                              int K, int32_t cols, int64_t elems, hipStream_t st, LaunchEv ev) {
    const int64_t nvec = elems / 4;
    if (nvec <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((nvec + 511) / 512);
    return launch_k(delta ? k_dense_floor<true> : k_dense_floor<false>, dim3(grid), dim3(256), 0, st, ev, data, out,
                    delta, bt, nb, stride, K, cols, nvec);
}

hipError_t launch_stream(bool copy, void* dst, const void* src, int64_t n16, hipStream_t st, LaunchEv ev) {
    if (n16 <= 0) return hipSuccess;
    const int64_t want = (n16 + 1023) / 1024;  // one 256-thread block per 4 wave steps
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, 256 * 16));
    return launch_k(copy ? k_stream<true> : k_stream<false>, dim3(grid), dim3(256), 0, st, ev, (uint8_t*)dst,
                    (const uint8_t*)src, n16);
}


}  // namespace dml

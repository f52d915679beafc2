// dml_ops.hip — the small kernels of a store's operations beside the push reduce: none
// is a hot path, each is one grid-stride loop.
//
//   k_array_rollback  int32 array stores: undo every add after the first negative
//                     counter (IntArrayStore.java:97-113); the arrays' ordered
//                     scatter-add itself is the partition + leaf path of dml_sparse.hip
//   k_key_rows        the row of every record of a push, for the host's duplicate-row replay
//   k_fill            init (dml_store_io.hip)
//   k_apply_dense, k_apply_dense_i32chk  the owner apply after a reduce-scatter
//                     (IntMatrixStore.java:174-176 for the check; dml_store_owner.hip)
//   k_fetch           handleFetch's record encode, one thread per (key, column)
//                     (FloatMatrixStore.java:140-153; dml_store_io.hip; the vectorised
//                     stream is dml_fetch.hip)
//   k_bswap4, k_bswap8  checkpoint byte order (dml_store_io.hip)
//   k_rand_f32, k_rand_f64_rows  DataStore.rand() (FloatMatrixStore.java:46-47,
//                     DoubleMatrixStore.java:196-206). Their caller, dml_store_rand, lives
//                     in dml_store_diag.hip with the java.util.Random model; rand() is a
//                     store operation, so the kernels are here and not in dml_diag.hip
//
// Driven by dml_store.hip (rollback, key rows), dml_store_io.hip, dml_store_owner.hip and
// dml_store_diag.hip as named above.
#include "dml_device.h"
#include "dml_launch.h"

namespace dml {

// ---------------------------------------------------------------------------
// Array stores (int32): undo after the first negative counter. Records
// [key][value] at stride K+VS; the ordered apply itself is the sorted leaf path
// (dml_sparse.hip).
// Undo (mod 2^32) every int32 array add positioned after the first negative.
__global__ __launch_bounds__(256) void k_array_rollback(int32_t* __restrict__ shard, int64_t rows,
                                                        const uint8_t* __restrict__ base, int64_t nrec, int b_global,
                                                        int64_t stride, int K, int64_t first, Ctrl* __restrict__ ctrl,
                                                        uint64_t tail_cut) {
    const uint64_t neg = ctrl->neg_pos;
    if (neg == kNoPos) return;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    uint64_t cut = ctrl->cutoff;
    if (tail_cut < cut) cut = tail_cut;
    const int64_t off = r * stride;
    if (pos_of((uint64_t)b_global, (uint64_t)off) >= cut) return;
    if (pos_of((uint64_t)b_global, (uint64_t)(off + K)) <= neg) return;
    const int64_t idx = row_index(ld_key(base + off, K), first, rows);
    if (idx < 0) return;
    atomicSub(&shard[idx], (int32_t)ld32(base + off + K));
}

hipError_t launch_array_rollback_i32(int32_t* shard, int64_t rows, const uint8_t* base, int64_t nrec, int b_global,
                                     int64_t stride, int K, int64_t first, Ctrl* ctrl, uint64_t tail_cut,
                                     hipStream_t st) {
    if (nrec <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_array_rollback, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st, shard, rows, base,
                       nrec, b_global, stride, K, first, ctrl, tail_cut);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
template <typename T>
__global__ void k_fill(T* __restrict__ p, int64_t n, T v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = v;
}
hipError_t launch_fill(int vtype, void* p, int64_t n, double v, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (vtype == kF32) hipLaunchKernelGGL(k_fill<float>, dim3(grid_for(n)), dim3(256), 0, st, (float*)p, n, (float)v);
    else if (vtype == kI32) hipLaunchKernelGGL(k_fill<int32_t>, dim3(grid_for(n)), dim3(256), 0, st, (int32_t*)p, n, (int32_t)v);
    else hipLaunchKernelGGL(k_fill<double>, dim3(grid_for(n)), dim3(256), 0, st, (double*)p, n, v);
    return hipGetLastError();
}
hipError_t launch_fill_f32(float* p, int64_t n, float v, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill<float>, dim3(grid_for(n)), dim3(256), 0, st, p, n, v);
    return hipGetLastError();
}

// shard += src, element-wise (owner apply after a reduce-scatter).
template <typename T>
__global__ __launch_bounds__(256) void k_apply_dense(T* __restrict__ shard, const T* __restrict__ src, int64_t n) {
    constexpr int VEC = Elem<T>::VEC;
    const int64_t nvec = n / VEC;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        T a[VEC], b[VEC];
        unpack<T>(((const u32x4*)shard)[i], a);
        unpack<T>(((const u32x4*)src)[i], b);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = Elem<T>::add(a[e], b[e]);
        ((u32x4*)shard)[i] = pack<T>(a);
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n - nvec * VEC) shard[nvec * VEC + t] = Elem<T>::add(shard[nvec * VEC + t], src[nvec * VEC + t]);
}
// int32 owner apply with IntMatrixStore's negativity check on the final counters
// (IntMatrixStore.java:174-176): the first negative element (row-major) of the
// first failing apply is kept in *neg (sticky: kNoPos until then); once it is
// set, later applies are no-ops (the reference store stops at its exception).
__global__ __launch_bounds__(256) void k_apply_dense_i32chk(int32_t* __restrict__ shard, const int32_t* __restrict__ src,
                                                            int64_t n, unsigned long long* neg) {
    if (__atomic_load_n(neg, __ATOMIC_RELAXED) != kNoPos) return;
    const int64_t nvec = n / 4;
    unsigned long long first = kNoPos;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t a[4], b[4];
        unpack<int32_t>(((const u32x4*)shard)[i], a);
        unpack<int32_t>(((const u32x4*)src)[i], b);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = Elem<int32_t>::add(a[e], b[e]);
            if (a[e] < 0 && first == kNoPos) first = (unsigned long long)(4 * i + e);
        }
        ((u32x4*)shard)[i] = pack<int32_t>(a);
    }
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n - nvec * 4) {
        const int64_t j = nvec * 4 + t;
        const int32_t v = Elem<int32_t>::add(shard[j], src[j]);
        shard[j] = v;
        if (v < 0 && first == kNoPos) first = (unsigned long long)j;
    }
    if (first != kNoPos) atomicMin(neg, first);
}

// The owner apply runs beside the next call's pre-reduce: a grid
// that fills every free wave slot keeps the pre-reduce's next blocks from being
// placed (its waves need most of a SIMD's VGPRs). kApplyBlocks bounds it to two
// blocks per CU; it still moves a config-2 shard's 192 MB well inside one call.
constexpr unsigned kApplyBlocks = 512;

hipError_t launch_apply_dense_i32chk(int32_t* shard, const int32_t* src, int64_t n, unsigned long long* neg,
                                     hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_apply_dense_i32chk, dim3(kApplyBlocks), dim3(256), 0, st, shard, src, n, neg);
    return hipGetLastError();
}

hipError_t launch_apply_dense(int vtype, void* shard, const void* src, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned g = kApplyBlocks;
    if (vtype == kF32) hipLaunchKernelGGL(k_apply_dense<float>, dim3(g), dim3(256), 0, st, (float*)shard, (const float*)src, n);
    else if (vtype == kI32) hipLaunchKernelGGL(k_apply_dense<int32_t>, dim3(g), dim3(256), 0, st, (int32_t*)shard, (const int32_t*)src, n);
    else hipLaunchKernelGGL(k_apply_dense<double>, dim3(g), dim3(256), 0, st, (double*)shard, (const double*)src, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// handleFetch encode, dense-column layouts (FloatMatrixStore.java:140-153 etc.).
// One thread per (key, column). `value_slot` = bytes per column in the output
// record (4/8; 8 for AdaGrad value+alpha and FloatArrayStore's 8-byte slot).

// CHECK (dml_store_fetch_device's list form, whose keys no host loop has seen): a key outside
// [first, last] reads nothing and writes nothing; the lowest list index of one lands in *bad.
template <typename T, bool CHECK = false>
__global__ void k_fetch(const T* __restrict__ shard, const float* __restrict__ alpha, int32_t cols,
                        const int64_t* __restrict__ keys, int64_t key_lo, int64_t n, int64_t first,
                        uint8_t* __restrict__ out, int64_t rec, int K, int value_slot, int64_t last = 0,
                        unsigned long long* __restrict__ bad = nullptr) {
    const int64_t total = n * (int64_t)cols;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t / cols;
        const int32_t c = (int32_t)(t - j * cols);
        const int64_t key = keys ? keys[j] : key_lo + j;
        const int64_t idx = key - first;
        if constexpr (CHECK) {
            if (key < first || key > last) {
                if (c == 0) atomicMin(bad, (unsigned long long)j);
                continue;
            }
        }
        uint8_t* o = out + j * rec;
        if (c == 0) {
            st32(o, (uint32_t)key);
            if (K == 8) st32(o + 4, (uint32_t)((uint64_t)key >> 32));
        }
        uint8_t* v = o + K + (int64_t)c * value_slot;
        const T x = shard[idx * cols + c];
        if constexpr (sizeof(T) == 4) {
            st32(v, __builtin_bit_cast(uint32_t, x));
        } else {
            const uint64_t u = __builtin_bit_cast(uint64_t, x);
            st32(v, (uint32_t)u); st32(v + 4, (uint32_t)(u >> 32));
        }
        if (alpha) st32(v + 4, __float_as_uint(alpha[idx * cols + c]));
        else if (sizeof(T) == 4 && value_slot == 8) st32(v + 4, 0u);  // FloatArrayStore's zero pad
    }
}
hipError_t launch_fetch(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                        int64_t key_lo, int64_t n, int64_t first, uint8_t* out, int64_t rec, int K, int value_slot,
                        hipStream_t st) {
    const int64_t total = n * (int64_t)cols;
    if (total <= 0) return hipSuccess;
    const dim3 g(grid_for(total));
    if (vtype == kF32) hipLaunchKernelGGL(k_fetch<float>, g, dim3(256), 0, st, (const float*)shard, alpha, cols, keys, key_lo, n, first, out, rec, K, value_slot);
    else if (vtype == kI32) hipLaunchKernelGGL(k_fetch<int32_t>, g, dim3(256), 0, st, (const int32_t*)shard, alpha, cols, keys, key_lo, n, first, out, rec, K, value_slot);
    else hipLaunchKernelGGL(k_fetch<double>, g, dim3(256), 0, st, (const double*)shard, alpha, cols, keys, key_lo, n, first, out, rec, K, value_slot);
    return hipGetLastError();
}
hipError_t launch_fetch_checked(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                                int64_t n, int64_t first, int64_t last, uint8_t* out, int64_t rec, int K,
                                int value_slot, unsigned long long* bad, hipStream_t st) {
    const int64_t total = n * (int64_t)cols;
    if (total <= 0) return hipSuccess;
    const dim3 g(grid_for(total));
    if (vtype == kF32) hipLaunchKernelGGL((k_fetch<float, true>), g, dim3(256), 0, st, (const float*)shard, alpha, cols, keys, (int64_t)0, n, first, out, rec, K, value_slot, last, bad);
    else if (vtype == kI32) hipLaunchKernelGGL((k_fetch<int32_t, true>), g, dim3(256), 0, st, (const int32_t*)shard, alpha, cols, keys, (int64_t)0, n, first, out, rec, K, value_slot, last, bad);
    else hipLaunchKernelGGL((k_fetch<double, true>), g, dim3(256), 0, st, (const double*)shard, alpha, cols, keys, (int64_t)0, n, first, out, rec, K, value_slot, last, bad);
    return hipGetLastError();
}

// Big-endian <-> native byte swap (DataOutputStream.writeFloat/writeInt/writeDouble).
__global__ void k_bswap4(const uint32_t* __restrict__ s, uint32_t* __restrict__ d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = __builtin_bswap32(s[i]);
}
__global__ void k_bswap8(const uint64_t* __restrict__ s, uint64_t* __restrict__ d, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = __builtin_bswap64(s[i]);
}
hipError_t launch_bswap(int V, const void* src, void* dst, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (V == 4) hipLaunchKernelGGL(k_bswap4, dim3(grid_for(n)), dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, n);
    else hipLaunchKernelGGL(k_bswap8, dim3(grid_for(n)), dim3(256), 0, st, (const uint64_t*)src, (uint64_t*)dst, n);
    return hipGetLastError();
}

// DataStore.rand() distributions (dml_store_rand). f32: (a/100f - 0.5f)/cols,
// a uniform in 0..99, float arithmetic as in FloatMatrixStore.java:46-47.
// f64: one thread per row, |N(0,1)| (Box-Muller) then the row over its L2 norm
// (DoubleMatrixStore.java:196-206).
__global__ void k_rand_f32(float* p, int64_t n, int32_t cols, uint64_t s0) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(splitmix64_dev(s0 + (uint64_t)i) % 100u);
        p[i] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)a, 100.0f), 0.5f), (float)cols);
    }
}
__device__ inline double rand_abs_gauss(uint64_t h) {
    const double u1 = (double)((h >> 11) + 1) * 0x1p-53;                   // (0, 1]
    const double u2 = (double)(splitmix64_dev(h) >> 11) * 0x1p-53;          // [0, 1)
    return fabs(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}
__global__ void k_rand_f64_rows(double* p, int64_t rows, int32_t cols, uint64_t s0) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        double* row = p + r * cols;
        double sum = 0.0;
        for (int32_t j = 0; j < cols; ++j) {
            const double g = rand_abs_gauss(splitmix64_dev(s0 + (uint64_t)(r * cols + j)));
            row[j] = g;
            sum = __dadd_rn(sum, __dmul_rn(g, g));
        }
        sum = sqrt(sum);
        for (int32_t j = 0; j < cols; ++j) row[j] = __ddiv_rn(row[j], sum);
    }
}
hipError_t launch_rand(int vtype, void* p, int64_t rows, int32_t cols, uint64_t s0, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    if (vtype == kF32) hipLaunchKernelGGL(k_rand_f32, dim3(grid_for(rows * cols)), dim3(256), 0, st, (float*)p, rows * cols, cols, s0);
    else if (vtype == kF64) hipLaunchKernelGGL(k_rand_f64_rows, dim3(grid_for(rows)), dim3(256), 0, st, (double*)p, rows, cols, s0);
    return hipGetLastError();
}

// Row index of every record of one push (-1 outside the shard): the host's
// duplicate-row replay reads these to split the push into unique-row layers.
__global__ void k_key_rows(const uint8_t* __restrict__ base, int64_t nrec, int64_t stride, int K, int64_t first,
                           int64_t rows, int32_t* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (int64_t)gridDim.x * blockDim.x)
        out[r] = (int32_t)row_index(ld_key(base + r * stride, K), first, rows);
}
hipError_t launch_key_rows(const uint8_t* base, int64_t nrec, int64_t stride, int K, int64_t first, int64_t rows,
                           int32_t* out, hipStream_t st) {
    if (nrec <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_key_rows, dim3(grid_for(nrec)), dim3(256), 0, st, base, nrec, stride, K, first, rows, out);
    return hipGetLastError();
}

}  // namespace dml

// dml_device.h — device-side helpers shared by the kernel files: vector load types, wire
// decode (DataDesc.java:131-192), KeyRange indexOf, IEEE element adds, 16-B pack / unpack,
// the wave's LDS hand-over, AdaGrad's alpha and the maxDelta candidates. Not part of the
// public ABI.
#pragma once
#include "dml_internal.h"

namespace dml {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(4)));  // records are 4-byte aligned only
typedef int32_t i32x8 __attribute__((ext_vector_type(8)));
typedef uint64_t u64x8 __attribute__((ext_vector_type(8)));

// Loads through the global address space: bucket pointers come out of the
// kernarg table as generic pointers, and flat loads would force vmcnt(0)+lgkmcnt(0)
// waits (flat returns out of order).
#define DML_GLOBAL __attribute__((address_space(1)))
__device__ inline u32x4 ldg16(const uint8_t* p) { return *(const DML_GLOBAL u32x4_u*)(p); }
__device__ inline uint32_t ldg32(const uint8_t* p) { return *(const DML_GLOBAL uint32_t*)(p); }
// Streamed-once bucket bytes: non-temporal policy (no L2 retention).
__device__ inline u32x4 ldg16_nt(const uint8_t* p) {
    return __builtin_nontemporal_load((const DML_GLOBAL u32x4_u*)(p));
}
__device__ inline void stg16_nt(void* p, u32x4 v) { __builtin_nontemporal_store(v, (DML_GLOBAL u32x4_u*)(p)); }
__device__ inline void stg16(void* p, u32x4 v) { *(DML_GLOBAL u32x4_u*)(p) = v; }
// Write-through 16-B store (sc1: the line leaves the XCD's L2 at once), through a
// buffer descriptor based at a wave-uniform `base` (byte offset `off` < nbytes):
// rows a kernel writes last leave no dirty L2 lines for the kernel-end writeback
// that holds up the next dispatch on the stream (MI355X_MICROARCH.md, kernel boundary).
__device__ inline void stg16_wt(const void* base, uint32_t nbytes, uint32_t off, u32x4 v) {
    const uint64_t b = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(nbytes);
    void* ub = (void*)(((uint64_t)hi << 32) | lo);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(ub, (short)0, (int)n, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)off, 0, 16);
}

// Buffer resource over [base, base + nbytes) at a wave-uniform base, and its 16-B
// non-temporal load (aux 2 = nt): 32-bit per-lane offsets instead of 64-bit
// addresses, and an offset past nbytes reads zeros (the range check), so a masked
// lane needs no select.
__device__ inline __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, uint32_t nbytes) {
    const uint64_t b = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(nbytes);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0, (int)n, 0x00020000);
}
__device__ inline u32x4 ldb16_nt(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 2);
}
// A wave-uniform 64-bit value in scalar registers (the compiler then branches on it
// with scalar branches).
__device__ inline int64_t uni64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ inline uint64_t uni64(uint64_t v) { return (uint64_t)uni64((int64_t)v); }
constexpr uint32_t kBufOff = 0xFFFFFFF0u;  // an offset past any range: the load reads zeros

// Blocks are dealt to the 8 XCDs round robin (block b on XCD b % 8), each XCD with
// its own L2. xcd_block() renumbers them so that XCD x runs the x-th contiguous run
// of block indices, in dispatch order: neighbouring blocks' data meets in one L2.
// A bijection on [0, gridDim.x) for any grid size.
__device__ inline int64_t xcd_block() {
    const int64_t nbk = gridDim.x, b = blockIdx.x, per = (nbk + 7) / 8, x = b % 8, i = b / 8;
    const int64_t full = nbk - (per - 1) * 8;  // XCDs 0..full-1 hold `per` blocks, the others per - 1
    return x < full ? x * per + i : full * per + (x - full) * (per - 1) + i;
}

__device__ inline uint32_t ld32(const uint8_t* p) { return ldg32(p); }
__device__ inline int64_t ld_key(const uint8_t* p, int K) {
    // DataDesc.readKey (DataDesc.java:131-138): LE int32 sign-extended, or LE int64.
    if (K == 4) return (int64_t)(int32_t)ld32(p);
    return (int64_t)((uint64_t)ld32(p) | ((uint64_t)ld32(p + 4) << 32));
}
// KeyRange indexOf: (int)(key - firstKey) (FloatMatrixStore.java:176-179); -1 if
// localData[index] would throw ArrayIndexOutOfBoundsException.
__device__ inline int64_t row_index(int64_t key, int64_t first, int64_t rows) {
    int32_t idx = (int32_t)(uint32_t)((uint64_t)key - (uint64_t)first);
    return (idx < 0 || (int64_t)idx >= rows) ? -1 : (int64_t)idx;
}

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int VEC = 4;
    __device__ static float from_bits(uint32_t lo, uint32_t) { return __uint_as_float(lo); }
    __device__ static float load(const uint8_t* p) { return __uint_as_float(ld32(p)); }
    __device__ static float add(float a, float b) { return __fadd_rn(a, b); }
};
template <> struct Elem<int32_t> {
    static constexpr int VEC = 4;
    __device__ static int32_t from_bits(uint32_t lo, uint32_t) { return (int32_t)lo; }
    __device__ static int32_t load(const uint8_t* p) { return (int32_t)ld32(p); }
    __device__ static int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
};
template <> struct Elem<double> {
    static constexpr int VEC = 2;
    __device__ static double from_bits(uint32_t lo, uint32_t hi) {
        return __longlong_as_double((long long)((uint64_t)lo | ((uint64_t)hi << 32)));
    }
    __device__ static double load(const uint8_t* p) { return from_bits(ld32(p), ld32(p + 4)); }
    __device__ static double add(double a, double b) { return __dadd_rn(a, b); }
};

// One 16-B vector <-> its VEC elements.
template <typename T>
__device__ inline void unpack(const u32x4& r, T* o) {
    if constexpr (sizeof(T) == 4) {
        o[0] = Elem<T>::from_bits(r.x, 0); o[1] = Elem<T>::from_bits(r.y, 0);
        o[2] = Elem<T>::from_bits(r.z, 0); o[3] = Elem<T>::from_bits(r.w, 0);
    } else {
        o[0] = Elem<T>::from_bits(r.x, r.y); o[1] = Elem<T>::from_bits(r.z, r.w);
    }
}
template <typename T>
__device__ inline u32x4 pack(const T* v) {
    u32x4 r;
    if constexpr (sizeof(T) == 4) {
        r.x = __builtin_bit_cast(uint32_t, v[0]); r.y = __builtin_bit_cast(uint32_t, v[1]);
        r.z = __builtin_bit_cast(uint32_t, v[2]); r.w = __builtin_bit_cast(uint32_t, v[3]);
    } else {
        uint64_t a = __builtin_bit_cast(uint64_t, v[0]), b = __builtin_bit_cast(uint64_t, v[1]);
        r.x = (uint32_t)a; r.y = (uint32_t)(a >> 32); r.z = (uint32_t)b; r.w = (uint32_t)(b >> 32);
    }
    return r;
}
__device__ inline void st32(uint8_t* p, uint32_t v) { *(uint32_t*)p = v; }

__host__ __device__ inline uint64_t splitmix64_dev(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A wave's LDS hand-over: what its lanes stored before is what any lane loads after.
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// AdaGrad's alpha of an element whose delta d ended above 1
// (FloatMatrixStoreAdaGrad.java:268-272): one double divide and sqrt, rounded to float,
// then the clamp. (The element step beside it, acc += g; delta += g*g with its last strict
// rise, stays written out in k_reduce's apply, k_ada_flat's upd, k_ada_ident and the two
// k_chain_ada_* steps: as a function, by reference or by value, inlined early or late, it
// changed the register allocation or the operand order of every one of them.)
__device__ __forceinline__ float ada_alpha(float d, float initial_alpha, float factor, float min_alpha) {
    const float a = (float)((double)initial_alpha / ((double)factor * sqrt((double)d)));
    return a < min_alpha ? min_alpha : a;
}

// maxDelta candidates: (valid, value, position), best = largest value,
// then smallest position (the first in the reference's order). Associative, so
// a block reduces them as a butterfly inside each wave, then across its waves
// through LDS; the result lands in thread 0. Every thread of the block calls it.
__device__ inline bool cand_better(bool ok, float v, uint64_t p, bool ok2, float v2, uint64_t p2) {
    return ok && (!ok2 || v > v2 || (v == v2 && p < p2));
}
template <int WPB>
__device__ inline void cand_block_best(bool& ok, float& v, uint64_t& p) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(v, m);
        const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)p, m);
        const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(p >> 32), m);
        const bool ook = __shfl_xor((int)ok, m) != 0;
        const uint64_t op = (uint64_t)olo | ((uint64_t)ohi << 32);
        if (cand_better(ook, ov, op, ok, v, p)) { ok = true; v = ov; p = op; }
    }
    if constexpr (WPB > 1) {
        __shared__ float sv[WPB];
        __shared__ uint64_t sp[WPB];
        __shared__ int sok[WPB];
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { sv[w] = v; sp[w] = p; sok[w] = ok; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 1; i < WPB; ++i)
                if (cand_better(sok[i] != 0, sv[i], sp[i], ok, v, p)) { ok = true; v = sv[i]; p = sp[i]; }
    }
}
// The best of cand[i], cand[i + step], ... below n, folded into (ok, v, p).
__device__ inline void cand_scan(const DeltaCand* __restrict__ cand, int64_t i, int64_t n, int64_t step, bool& ok,
                                 float& v, uint64_t& p) {
    for (; i < n; i += step) {
        const DeltaCand c = cand[i];
        if (cand_better(c.valid != 0, c.value, c.pos, ok, v, p)) { ok = true; v = c.value; p = c.pos; }
    }
}
// The candidate as a block's thread 0 stores it (after cand_block_best).
__device__ __forceinline__ DeltaCand cand_of(const bool& ok, const float& v, const uint64_t& p) {
    DeltaCand c;
    c.value = v; c.valid = ok; c.pos = p;
    return c;
}

}  // namespace dml

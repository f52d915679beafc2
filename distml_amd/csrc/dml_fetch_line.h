// dml_fetch_line.h — the line walk of the record-encode kernels: k_fetch_vec
// (dml_fetch.hip) and k_rec_pack (dml_codec.hip, §4.12). One thread
// owns one 16-byte line of the output ADDRESS: it finds the record its first dword
// falls in, then walks its four dwords through at most three records. The two kernels
// differ only in where record j's row comes from (ROWS), so the walk exists once.
// Device only; not part of the public ABI.
#pragma once
#include "dml_device.h"

namespace dml {

constexpr int kPlain = 0;  // values are the row's dwords in order (f32, i32, f64 matrices and arrays)
constexpr int kAda = 1;    // [value][alpha] pairs (FloatMatrixStoreAdaGrad)
constexpr int kPad = 2;    // [value][0] (FloatArrayStore's 8-byte slot)

constexpr int kRowOfKey = 0;     // a shard: record j is row key - first, a key outside [first, last] is refused
constexpr int kRowOfRecord = 1;  // a dense T[n][cols] buffer: record j is row j, no key is refused

struct FetchP {
    const uint32_t* data;   // the rows, as dwords
    const uint32_t* alpha;  // kAda
    const int64_t* keys;    // null: key = key_lo + record index
    int64_t key_lo, first, last;  // first, last: kRowOfKey
    uint8_t* line0;         // dev_out rounded down to 16 bytes
    int64_t ndw;            // dwords of the stream
    int64_t rowdw;          // dwords of one row (cols x V / 4)
    int32_t cols, recdw, kdw, lead;
    unsigned long long* bad;  // kRowOfKey
};

__device__ inline void stg32_nt(void* p, uint32_t v) { __builtin_nontemporal_store(v, (DML_GLOBAL uint32_t*)p); }
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_u __attribute__((aligned(4)));
__device__ inline u32x2 ldg8(const uint32_t* p) { return *(const DML_GLOBAL u32x2_u*)p; }

// WIDE: the record of a line by 64-bit division whatever the stream's length (the path
// streams of 2^32 dwords and more take; a diagnostic switch runs it on small ones).
template <int LAYOUT, bool VLOAD, int ROWS = kRowOfKey, bool WIDE = false>
__device__ inline void fetch_line(const FetchP& a, int64_t v) {
    const int64_t d0 = 4 * v - a.lead;  // stream dword of the line's first slot (< 0 only on line 0)
    const int64_t lo = d0 < 0 ? 0 : d0;
    const int64_t hi = d0 + 4 < a.ndw ? d0 + 4 : a.ndw;
    if (lo >= hi) return;
    int64_t j;
    // narrowed: lo < ndw <= 2^32 - 1 and recdw < 2^31, so both fit a uint32
    if (!WIDE && a.ndw <= 0xFFFFFFFFll) j = (int64_t)((uint32_t)lo / (uint32_t)a.recdw);
    else j = lo / a.recdw;
    int32_t w = (int32_t)(lo - j * a.recdw);  // dword inside record j

    int64_t key = a.keys ? a.keys[j] : a.key_lo + j;
    bool good = ROWS == kRowOfRecord || (key >= a.first && key <= a.last);
    int64_t idx = ROWS == kRowOfRecord ? j : key - a.first;

    if (good && w >= a.kdw && w + 4 <= a.recdw && hi - lo == 4) {
        const int32_t c = w - a.kdw;
        if (LAYOUT == kPlain && VLOAD) {
            stg16_nt(a.line0 + 16 * v, ldg16((const uint8_t*)(a.data + idx * a.rowdw + c)));
            return;
        }
        if (LAYOUT == kAda && VLOAD && (c & 1) == 0) {
            const int64_t e = idx * a.cols + (c >> 1);
            const u32x2 x = ldg8(a.data + e), al = ldg8(a.alpha + e);
            u32x4 o;
            o.x = x.x; o.y = al.x; o.z = x.y; o.w = al.y;
            stg16_nt(a.line0 + 16 * v, o);
            return;
        }
    }

    uint32_t val[4] = {0u, 0u, 0u, 0u};
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t d = d0 + e;
        if (d < lo || d >= hi) continue;
        if (w == a.recdw) {
            w = 0;
            ++j;
            key = a.keys ? a.keys[j] : a.key_lo + j;
            good = ROWS == kRowOfRecord || (key >= a.first && key <= a.last);
            idx = ROWS == kRowOfRecord ? j : key - a.first;
        }
        if (!good) {
            if (w == 0) atomicMin(a.bad, (unsigned long long)j);
        } else {
            uint32_t x;
            if (w < a.kdw) {
                x = w == 0 ? (uint32_t)key : (uint32_t)((uint64_t)key >> 32);
            } else {
                const int32_t c = w - a.kdw;
                if (LAYOUT == kPlain) x = a.data[idx * a.rowdw + c];
                else if (LAYOUT == kAda) x = (c & 1) ? a.alpha[idx * a.cols + (c >> 1)] : a.data[idx * a.cols + (c >> 1)];
                else x = (c & 1) ? 0u : a.data[idx];
            }
            val[e] = x;
            mask |= 1u << e;
        }
        ++w;
    }
    uint8_t* o = a.line0 + 16 * v;
    if (mask == 0xFu) {
        u32x4 q;
        q.x = val[0]; q.y = val[1]; q.z = val[2]; q.w = val[3];
        stg16_nt(o, q);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (mask & (1u << e)) stg32_nt(o + 4 * e, val[e]);
    }
}

}  // namespace dml

// dml_fetch_compact.hip — the compact fetch of int32 rows: the fetch half of
// the route whose push half is dml_compact_rows.hip (§4.19). LightLDA's word-topic rows are mostly
// zeros, and a dense fetch record is 4 x cols bytes per word however few topics hold a count; a
// compact row is 8 bytes per non-zero counter. Two endpoints, no transport:
//
// Owner (dml_store_fetch_compact_rows_device), on the store's apply stream, no host wait:
//   k_cf_rows<false>   the count pass. An item is (list index j, slice of kCfSlice dwords of the
//                 row of keys[j]), one wave per item, the slice IN REGISTERS: lane l issues the
//                 16-byte cached loads of vectors r x 64 + l, r = 0 .. 3, before the first ballot;
//                 no LDS. A row's ragged last vector is loaded shifted back to end at the row's
//                 last byte and its trailing dwords moved to the front (k_fetch_planes' rule); a
//                 row of 1 .. 3 dwords is lane 0's dword loads. Dwords past the row are zero, and a
//                 zero is no entry, so nothing below knows about edges. Per round one ballot per
//                 dword component; their popcounts add up to cnt[j x nslice + slice]. A key outside
//                 [first, last] (64-bit compare) is never turned into an address: its items count
//                 zero and its list index goes to `bad` by atomicMin (k_fetch_verdict's input).
//   k_cr_scan     dml_compact_rows.hip's, as it is: cnt[] to its exclusive running sum, ptr[j] =
//                 the sum in front of key j's first slice, ptr[n] = cnt[n x nslice] = the total.
//   k_cf_rows<true>    the writing pass. It reads the total first: above the capacity, no thread
//                 stores anything. The rows are RE-READ, not kept: a kept copy is the dense plane
//                 this form exists to avoid (§4.19's argument for rebuilding slices); an item whose
//                 count is zero is not read again. The column order of a round is lane-major,
//                 component-minor, so a non-zero dword's rank is the popcounts of the four ballots
//                 below the lane plus the lane's own earlier non-zero components, and its position
//                 cnt[item] + the non-zeros of the rounds before + that rank: a sum of counts, no
//                 atomic decides one, two runs give equal bytes and the columns of a row ascend.
//                 Entries leave by non-temporal dword stores. A repeated key re-reads its row
//                 through L2, as in k_fetch_planes.
//
// Requester (dml_compact_rows_expand_device), store-less, on the caller's stream:
//   k_cf_expand   one wave per (occurrence j, slice) with a private 4-KiB LDS slice: zero it, walk
//                 the entries of compact row inverse[j] 64 at a time (the next batch's loads in
//                 flight over this batch's ds_add_u32), store the slice once with 16-byte
//                 non-temporal stores: the plane is written once, where a memset and a scatter
//                 would write it twice. The list may come from another rank: a row whose inverse
//                 entry or entry range is out of bounds is left untouched, a column outside
//                 [0, cols) adds nothing, repeated columns sum, no index at or past `entries` is
//                 read. There is no block route for long rows as the compact push has one: a
//                 canonical row has at most cols entries, a wave's walk of 16 batches per slice.
// No float op is in this file.
#include <algorithm>

#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kCfSlice = DML_COALESCE_ELEMS_SLICE;  // dwords of a row that one item holds
constexpr int kCfWaves = kCoBlock / 64;
constexpr int kCfVec = kCfSlice / 4 / 64;            // 16-byte vectors of a slice per lane: the rounds
constexpr int64_t kCfMaxBlocks = (int64_t)1 << 22;
static_assert(kCfVec * 256 == kCfSlice && kCfWaves * kCfSlice * 4 <= 65536,
              "a lane holds whole vectors of its slice; a block's slices fit LDS");

// Vector v of the slice of w dwords at `p`, dwords past the slice's end zero. `tail`: the row is
// 16 bytes and more, so its ragged last vector is one load that ends at the row's last byte.
__device__ inline u32x4 slice_vec(const uint8_t* p, uint32_t v, uint32_t w, bool tail) {
    u32x4 x = {0u, 0u, 0u, 0u};
    const uint32_t d0 = 4 * v;
    if (d0 + 4 <= w) return ldg16(p + 16 * v);
    if (d0 >= w) return x;
    const uint32_t keep = w - d0;  // 1 .. 3
    if (tail) {
        const u32x4 t = ldg16(p + 4 * (int64_t)w - 16);
        if (keep == 3) { x.x = t.y; x.y = t.z; x.z = t.w; }
        else if (keep == 2) { x.x = t.z; x.y = t.w; }
        else x.x = t.w;
        return x;
    }
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d)
        if (d < keep) x[d] = ldg32(p + 16 * v + 4 * d);
    return x;
}

template <bool WRITE>
__global__ __launch_bounds__(kCoBlock) void k_cf_rows(const FetchCompactP a) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t nitem = a.n * a.nslice;
    uint32_t total = 0;
    if constexpr (WRITE) {
        total = a.cnt[nitem];
        if ((unsigned long long)total > (unsigned long long)a.cap) return;  // ptr[n] tells the caller
    }
    for (int64_t item = (int64_t)blockIdx.x * kCfWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kCfWaves) {
        const int64_t j = a.nslice == 1 ? item : item / a.nslice;
        const uint32_t c0 = (uint32_t)(item - j * a.nslice) * kCfSlice;
        const uint32_t w = (uint32_t)a.cols - c0 < (uint32_t)kCfSlice ? (uint32_t)a.cols - c0 : (uint32_t)kCfSlice;
        uint32_t base = 0;
        if constexpr (WRITE) {
            base = a.cnt[item];
            if (a.cnt[item + 1] == base) continue;  // no entry: the slice is not read again
        }
        int32_t mine = -1;
        if (lane == 0) {
            const int64_t key = a.keys[j];
            if (key >= a.first && key <= a.last) mine = (int32_t)(key - a.first);  // rows <= INT32_MAX
            else if (!WRITE && c0 == 0) atomicMin(a.bad, (unsigned long long)j);
        }
        const int32_t row = __builtin_amdgcn_readfirstlane(mine);
        if (row < 0) {
            if constexpr (!WRITE) {
                if (lane == 0) a.cnt[item] = 0u;
            }
            continue;
        }
        const uint8_t* p = (const uint8_t*)a.data + ((int64_t)row * a.cols + c0) * 4;
        u32x4 x[kCfVec];  // every load before the first ballot
#pragma unroll
        for (int r = 0; r < kCfVec; ++r) {
            x[r] = u32x4{0u, 0u, 0u, 0u};
            if ((uint32_t)r * 256u < w) x[r] = slice_vec(p, (uint32_t)r * 64u + lane, w, a.cols >= 4);
        }
#pragma unroll
        for (int r = 0; r < kCfVec; ++r) {
            if ((uint32_t)r * 256u >= w) break;
            const unsigned long long b0 = __ballot(x[r].x != 0u), b1 = __ballot(x[r].y != 0u);
            const unsigned long long b2 = __ballot(x[r].z != 0u), b3 = __ballot(x[r].w != 0u);
            if constexpr (WRITE) {
                uint32_t pos = base + (uint32_t)(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) +
                                                 __popcll(b3 & below));
                const uint32_t col = c0 + 4u * ((uint32_t)r * 64u + lane);
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d) {
                    // pos < total by construction (both passes read the same rows); the compare
                    // keeps a count that disagrees from ever becoming a store outside the arrays
                    if (x[r][d] != 0u && pos < total) {
                        stg32_nt(a.ecol + pos, col + d);
                        stg32_nt(a.eval + pos, x[r][d]);
                        ++pos;
                    }
                }
            }
            base += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        }
        if constexpr (!WRITE) {
            if (lane == 0) a.cnt[item] = base;
        }
    }
}

struct ExpandCompactP {
    const int32_t* ptr;   // int32[m + 1]
    const int32_t* ecol;  // int32[entries]
    const int32_t* eval;
    const int32_t* inv;   // int32[n], null: the identity
    uint8_t* plane;       // int32[n][cols], 4-byte aligned
    int64_t m, entries, n;
    int64_t nslice;
    int32_t cols;
};

__global__ __launch_bounds__(kCoBlock) void k_cf_expand(const ExpandCompactP a) {
    __shared__ u32x4 lds[kCfWaves][kCfSlice / 4];
    const uint32_t lane = threadIdx.x & 63;
    uint32_t* sl = (uint32_t*)lds[threadIdx.x >> 6];
    const int64_t nitem = a.n * a.nslice;
    for (int64_t item = (int64_t)blockIdx.x * kCfWaves + (threadIdx.x >> 6); item < nitem;
         item += (int64_t)gridDim.x * kCfWaves) {
        const int64_t j = a.nslice == 1 ? item : item / a.nslice;
        const uint32_t c0 = (uint32_t)(item - j * a.nslice) * kCfSlice;
        const uint32_t w = (uint32_t)a.cols - c0 < (uint32_t)kCfSlice ? (uint32_t)a.cols - c0 : (uint32_t)kCfSlice;
        // the row's range, or an empty one at -1 for a row that stays untouched: wave-uniform
        int32_t s0 = -1, e0 = -1;
        if (lane == 0) {
            const int64_t u = a.inv ? (int64_t)a.inv[j] : j;
            if (u >= 0 && u < a.m) {
                const int32_t ps = a.ptr[u], pe = a.ptr[u + 1];
                if (ps >= 0 && ps <= pe && (int64_t)pe <= a.entries) {
                    s0 = ps;
                    e0 = pe;
                }
            }
        }
        const int32_t sr = __builtin_amdgcn_readfirstlane(s0), er = __builtin_amdgcn_readfirstlane(e0);
        if (sr < 0) continue;
        const uint32_t s = (uint32_t)sr, e = (uint32_t)er;
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
        uint8_t* p = a.plane + (j * a.cols + c0) * 4;
#pragma unroll
        for (int k = 0; k < kCfVec; ++k) {
            const uint32_t v = lane + 64 * k;
            if (4 * v >= w) continue;
            const u32x4 x = ((const u32x4*)sl)[v];
            if (4 * v + 4 <= w) stg16_nt(p + 16 * v, x);
            else store_vec(p, v, w, x);  // the row's ragged tail, dword by dword
        }
        wave_phase();  // the next item's zeroing comes after this read-back
    }
}

bool overlap(const void* a, int64_t alen, const void* b, int64_t blen) {
    if (!a || !b || alen <= 0 || blen <= 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)blen && y < x + (uintptr_t)alen;
}

}  // namespace

hipError_t launch_fetch_compact(const FetchCompactP& a, hipStream_t st) {
    const int64_t nitem = a.n * a.nslice;
    const unsigned blocks = (unsigned)std::min<int64_t>((nitem + kCfWaves - 1) / kCfWaves, kCfMaxBlocks);
    hipLaunchKernelGGL((k_cf_rows<false>), dim3(blocks), dim3(kCoBlock), 0, st, a);
    launch_compact_scan(a.cnt, nitem, a.nslice, a.ptr, st);
    hipLaunchKernelGGL((k_cf_rows<true>), dim3(blocks), dim3(kCoBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace dml

using namespace dml;

extern "C" int dml_compact_rows_expand_device(const int32_t* dev_ptr, const int32_t* dev_ecol, const int32_t* dev_eval,
                                              int64_t m, int64_t entries, int32_t cols, const int32_t* dev_inverse,
                                              int64_t n, int32_t* dev_plane_out, void* stream) {
    // ---- argument checks: no HIP call before they pass
    if (m < 0 || n < 0 || entries < 0) return set_error(DML_E_INVALID_ARG, "negative row, entry or occurrence count");
    if (cols <= 0) return set_error(DML_E_INVALID_ARG, "cols must be > 0");
    if (m > 0x7FFFFFFFll || n > 0x7FFFFFFFll) return set_error(DML_E_INVALID_ARG, "lists of 2^31 rows and more");
    if (!dev_inverse && n != m) return set_error(DML_E_INVALID_ARG, "a null inverse is the identity: n must equal m");
    if ((((uintptr_t)dev_ptr | (uintptr_t)dev_ecol | (uintptr_t)dev_eval | (uintptr_t)dev_inverse |
          (uintptr_t)dev_plane_out) & 3u) != 0)
        return set_error(DML_E_INVALID_ARG, "ptr, entries, inverse or plane pointer is not 4-byte aligned");
    if ((n > 0 && !dev_plane_out) || (m > 0 && !dev_ptr) || (entries > 0 && (!dev_ecol || !dev_eval)))
        return set_error(DML_E_INVALID_ARG, "null plane, ptr or entries pointer");
    if (n > INT64_MAX / ((int64_t)cols * 4)) return set_error(DML_E_INVALID_ARG, "the plane's byte length overflows");
    const int64_t pbytes = n * cols * 4;
    const void* in[4] = {dev_ptr, dev_ecol, dev_eval, dev_inverse};
    const int64_t inlen[4] = {m > 0 ? (m + 1) * 4 : 0, entries * 4, entries * 4, dev_inverse ? n * 4 : 0};
    for (int i = 0; i < 4; ++i)
        if (overlap(dev_plane_out, pbytes, in[i], inlen[i]))
            return set_error(DML_E_INVALID_ARG, "expand output overlaps an input");
    if (n == 0 || m == 0) return DML_OK;  // no entry of the inverse names a row: every plane row stays as it is
    ExpandCompactP a;
    a.ptr = dev_ptr;
    a.ecol = dev_ecol;
    a.eval = dev_eval;
    a.inv = dev_inverse;
    a.plane = (uint8_t*)dev_plane_out;
    a.m = m;
    a.entries = entries;
    a.n = n;
    a.nslice = ((int64_t)cols + kCfSlice - 1) / kCfSlice;
    a.cols = cols;
    const int64_t nitem = n * a.nslice;
    const unsigned blocks = (unsigned)std::min<int64_t>((nitem + kCfWaves - 1) / kCfWaves, kCfMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cf_expand, dim3(blocks), dim3(kCoBlock), 0, st, a);
    HIPCHK(hipGetLastError());
    if (!st) HIPCHK(hipStreamSynchronize(st));
    return DML_OK;
}

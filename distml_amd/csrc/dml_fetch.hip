// dml_fetch.hip — the record encode of dml_store_fetch_device.
//
// handleFetch's dense-column layouts (FloatMatrixStore.java:113-174,
// IntMatrixStore.java:81-140, DoubleMatrixStore.java:80-139,
// FloatMatrixStoreAdaGrad.java:146-213, FloatArrayStore.java:88-108,
// IntArrayStore.java:78-95, DoubleArrayStore.java:93-113) as ONE packed stream of
// nkeys records, written in whole 16-byte vectors.
//
// k_fetch_vec is output-stationary. The stream is cut at the 16-byte lines of the
// output ADDRESS (dev_out is 4-byte aligned only: `lead` dwords of the first line lie
// before it), and one thread owns one such line: it finds the record its first dword
// falls in (one division per line, 32-bit when the stream is under 2^32 dwords), then
// walks its four dwords through at most three records. With records of kFetchVloadMinDw
// dwords or more, a line inside one record's values of a plain store is one
// 4-byte-aligned 16-byte load of the shard, and AdaGrad's [value][alpha] pairs are two
// 8-byte loads interleaved in registers; every other line (one with a key, a record
// boundary, FloatArrayStore's zero pad, and every line of shorter records) gathers its
// dwords singly. All four dwords leave in one non-temporal 16-byte store; only the
// stream's first and last line, and a line that touches a refused record, fall back
// to single dwords. Bytes pass through as uint32: no float instruction touches them.
//
// A key is loaded once per record a line touches (the range form computes it). A key
// outside [first, last] is never turned into an address: its record's dwords are
// skipped, and the thread that owns the record's first dword reports the list index.
// The walk itself (fetch_line) is dml_fetch_line.h, shared with k_rec_pack.
#include "dml_fetch_line.h"

namespace dml {

namespace {

// U lines per thread, a block's U x 256 lines contiguous, one wave instruction's 64 lines
// contiguous (DML_FETCH_WAVE_BYTES; DML_FETCH_BLOCK_BYTES is the shipped U = 1). Blocks run
// in dispatch order: xcd_block() numbering measured 1.5-3 % slower here.
template <int LAYOUT, bool VLOAD, bool XCD, int U>
__global__ __launch_bounds__(256) void k_fetch_vec(const FetchP a, int64_t nline) {
    const int64_t blk = XCD ? xcd_block() : (int64_t)blockIdx.x;
    const int64_t v0 = blk * (256 * U) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t v = v0 + u * 256;
        if (v < nline) fetch_line<LAYOUT, VLOAD>(a, v);
    }
}

__global__ void k_fetch_verdict(unsigned long long* bad, const int64_t* keys, FetchVerdict* v) {
    const unsigned long long i = *bad;
    if (i == kNoPos) return;
    if (v->idx == kNoPos) {
        v->key = keys[i];
        v->idx = i;
    }
    *bad = kNoPos;
}

template <int LAYOUT, bool VLOAD, bool XCD, int U>
void launch_t(const FetchP& a, int64_t nline, hipStream_t st) {
    const int64_t per = 256 * U;
    hipLaunchKernelGGL((k_fetch_vec<LAYOUT, VLOAD, XCD, U>), dim3((unsigned)((nline + per - 1) / per)), dim3(256), 0, st,
                       a, nline);
}
// Records of at least this many dwords take the 16-byte shard loads; shorter ones gather
// every dword singly (with a record boundary in every wave both paths of
// the load run in every wave, and the single path is the faster one).
constexpr int32_t kFetchVloadMinDw = 768;
constexpr bool kFetchOnePerThread = true;   // the shipped lines per thread: 1, or 4

template <int LAYOUT>
void launch_l(const FetchP& a, int64_t nline, int variant, hipStream_t st) {
    const int mode = variant & kFetchVarLoadMask;
    const bool vload = mode == kFetchVarVload || (mode == 0 && a.recdw >= kFetchVloadMinDw);
    const bool xcd = (variant & kFetchVarXcd) != 0;
    const bool u1 = (variant & kFetchVarU1) != 0 || (kFetchOnePerThread && (variant & kFetchVarU4) == 0);
    switch ((vload ? 1 : 0) | (xcd ? 2 : 0) | (u1 ? 4 : 0)) {
        case 0: return launch_t<LAYOUT, false, false, 4>(a, nline, st);
        case 1: return launch_t<LAYOUT, true, false, 4>(a, nline, st);
        case 2: return launch_t<LAYOUT, false, true, 4>(a, nline, st);
        case 3: return launch_t<LAYOUT, true, true, 4>(a, nline, st);
        case 4: return launch_t<LAYOUT, false, false, 1>(a, nline, st);
        case 5: return launch_t<LAYOUT, true, false, 1>(a, nline, st);
        case 6: return launch_t<LAYOUT, false, true, 1>(a, nline, st);
        default: return launch_t<LAYOUT, true, true, 1>(a, nline, st);
    }
}

}  // namespace

hipError_t launch_fetch_vec(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                            int64_t key_lo, int64_t n, int64_t first, int64_t last, uint8_t* out, int64_t rec, int K,
                            int value_slot, unsigned long long* bad, int variant, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int V = vtype == kF64 ? 8 : 4;
    FetchP a;
    a.data = (const uint32_t*)shard;
    a.alpha = (const uint32_t*)alpha;
    a.keys = keys;
    a.key_lo = key_lo;
    a.first = first;
    a.last = last;
    a.lead = (int32_t)(((uintptr_t)out & 15) >> 2);
    a.line0 = out - 4 * a.lead;
    a.ndw = n * (rec / 4);
    a.rowdw = (int64_t)cols * (V / 4);
    a.cols = cols;
    a.recdw = (int32_t)(rec / 4);
    a.kdw = K / 4;
    a.bad = bad;
    const int64_t nline = (a.ndw + a.lead + 3) / 4;
    if (alpha) launch_l<kAda>(a, nline, variant, st);
    else if (value_slot != V) launch_l<kPad>(a, nline, variant, st);
    else launch_l<kPlain>(a, nline, variant, st);
    return hipGetLastError();
}

hipError_t launch_fetch_verdict(unsigned long long* bad, const int64_t* keys, FetchVerdict* v, hipStream_t st) {
    hipLaunchKernelGGL(k_fetch_verdict, dim3(1), dim3(1), 0, st, bad, keys, v);
    return hipGetLastError();
}

}  // namespace dml

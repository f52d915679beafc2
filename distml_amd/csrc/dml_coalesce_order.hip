// dml_coalesce_order.hip — the coalescer's order stage for keys in a declared range
// (dml_coalescer_set_key_range): a stable LSD radix sort of 64-bit words
//
//     word = (key - first) << 32 | occurrence index          (rel = key - first < span <= 2^32)
//
// over the bits of span - 1 alone, in P = ceil(bits / kOrdBits) passes of near-equal digit
// widths. It ends where the library sort of dml_coalesce.hip ends: kout[i] = key ^ sign bit
// and vout[i] = occurrence index, ordered by key and, inside a key, by list position, which is
// all k_co_heads and the sum kernels read. A pass is three launches and no block ever waits
// for another:
//
//   k_ord_count    G = min(tiles, kOrdMaxBlocks) blocks. Block b owns a contiguous run of whole
//                  kOrdTile-word tiles and counts the run's digits in an LDS histogram (LDS
//                  atomics: counts commute), then stores count[digit][b]. <FIRST> reads the
//                  caller's int64 keys, so no pairs kernel exists on this route, and checks the
//                  range: a thread that meets rel >= span stores the call's epoch to the flag
//                  word beside the count word (plain stores, every writer the same value).
//   k_ord_scan     one block: the exclusive scan of the digits x G counts, digit-major, in
//                  place, so count[d][b] becomes where block b's first word of digit d goes.
//   k_ord_scatter  the same ownership. A block walks its run tile by tile with its per-digit
//                  bases in LDS. In a tile each of the four waves owns a contiguous quarter and
//                  takes it 64 consecutive words a round, so wave, round, lane is list order. A
//                  lane's rank among the equal digits of its round is a match: one __ballot per
//                  digit bit, the masks intersected, popcount below the lane. A per-wave
//                  per-digit running count in LDS carries the ranks from round to round (a
//                  wave's LDS operations complete in issue order). After one barrier thread d
//                  turns the four waves' counts of digit d into their starts inside the tile's
//                  sorted order; the words go to LDS at those places and leave for global memory
//                  position by position, a digit's words as one contiguous run.
//                  <LAST> writes kout / vout instead of words.
//
// No atomic decides a position, so two runs give equal bytes. A digit is masked to its width
// whatever the key, and every global store is checked against n: a key outside the range
// cannot make a kernel read or write out of bounds; it only raises the flag, and the host then
// orders the list again with the library sort.
#include "dml_coalesce_dev.h"

namespace dml {
namespace {

constexpr int kOrdBits = DML_COALESCE_ORDER_BITS;
constexpr int kOrdDigits = 1 << kOrdBits;
constexpr int kOrdTile = DML_COALESCE_ORDER_TILE;
constexpr int kOrdMaxBlocks = DML_COALESCE_ORDER_MAX_BLOCKS;
constexpr int kOrdWaves = kCoBlock / 64;
constexpr int kOrdPerThread = kOrdTile / kCoBlock;       // words of a tile per thread
constexpr int kOrdRounds = kOrdTile / kOrdWaves / 64;    // 64-word rounds of a wave's quarter
constexpr int kScanThreads = 1024, kScanRows = 16;
constexpr uint64_t kSignBit = 1ull << 63;
static_assert(kOrdDigits == kCoBlock, "thread d of a block owns digit d");
static_assert(kOrdRounds * kOrdWaves * 64 == kOrdTile && kOrdRounds == kOrdPerThread, "a tile is whole rounds of four waves");

struct Pass {
    const int64_t* keys;   // FIRST: the caller's keys
    const uint64_t* in;    // otherwise: the words the pass before wrote
    uint64_t* out;         // the words this pass writes, or (LAST) kout
    uint32_t* vout;        // LAST
    uint32_t* count;       // [digits][G]
    uint32_t* flag;        // FIRST
    int64_t n;
    uint64_t first, span;
    int64_t tiles;
    uint32_t epoch;
    int32_t shift, mask;   // this pass's digit of rel
};

// The tiles [t0, t1) of block b: the first tiles % G blocks own one tile more.
__device__ inline void own_tiles(int64_t tiles, int64_t* t0, int64_t* t1) {
    const int64_t G = gridDim.x, b = blockIdx.x, per = tiles / G, rem = tiles % G;
    *t0 = b * per + (b < rem ? b : rem);
    *t1 = *t0 + per + (b < rem ? 1 : 0);
}

__device__ inline uint32_t digit_of(uint64_t word, const Pass& a) {
    return ((uint32_t)(word >> 32) >> a.shift) & (uint32_t)a.mask;
}

// Word i of the pass's input, i < n. FIRST: made from key i, and the range check.
template <bool FIRST>
__device__ inline uint64_t word_at(const Pass& a, int64_t i) {
    if constexpr (FIRST) {
        const uint64_t rel = (uint64_t)a.keys[i] - a.first;
        if (rel >= a.span) *a.flag = a.epoch;
        return rel << 32 | (uint64_t)i;
    } else {
        return a.in[i];
    }
}

template <bool FIRST>
__global__ __launch_bounds__(kCoBlock) void k_ord_count(const Pass a) {
    __shared__ uint32_t hist[kOrdDigits];
    hist[threadIdx.x] = 0;
    __syncthreads();
    int64_t t0, t1;
    own_tiles(a.tiles, &t0, &t1);
    for (int64_t t = t0; t < t1; ++t) {
        uint64_t w[kOrdPerThread];
#pragma unroll
        for (int k = 0; k < kOrdPerThread; ++k) {
            const int64_t i = t * kOrdTile + k * kCoBlock + threadIdx.x;
            w[k] = i < a.n ? word_at<FIRST>(a, i) : 0;
        }
#pragma unroll
        for (int k = 0; k < kOrdPerThread; ++k) {
            const int64_t i = t * kOrdTile + k * kCoBlock + threadIdx.x;
            if (i < a.n) atomicAdd(&hist[digit_of(w[k], a)], 1u);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= a.mask) a.count[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = hist[threadIdx.x];
}

__device__ inline uint32_t wave_incl(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// count[0..total) to its exclusive running sum, in place. A step is kScanThreads x kScanRows
// counts: each wave takes a contiguous run of kScanRows x 64 of them, 64 consecutive counts a
// load, so loads and stores coalesce, and scans it by shuffles; one barrier joins the waves, and
// the carry goes from one step to the next (the shape of k_co_offsets).
__global__ __launch_bounds__(kScanThreads) void k_ord_scan(uint32_t* __restrict__ count, int64_t total) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (int64_t base = 0; base < total; base += kScanThreads * kScanRows) {
        const int64_t i0 = base + (int64_t)wave * (64 * kScanRows) + lane;
        uint32_t v[kScanRows];
#pragma unroll
        for (int e = 0; e < kScanRows; ++e) v[e] = i0 + e * 64 < total ? count[i0 + e * 64] : 0;
        uint32_t run = 0;  // the wave's counts before row e
#pragma unroll
        for (int e = 0; e < kScanRows; ++e) {
            const uint32_t incl = wave_incl(v[e]);
            v[e] = run + incl - v[e];
            run += (uint32_t)__shfl((int)incl, 63);
        }
        if (lane == 0) wsum[wave] = run;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
#pragma unroll
        for (int e = 0; e < kScanRows; ++e)
            if (i0 + e * 64 < total) count[i0 + e * 64] = before + v[e];
        carry += all;
        __syncthreads();  // wsum is rewritten by the next step
    }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kCoBlock) void k_ord_scatter(const Pass a) {
    __shared__ uint64_t sorted[kOrdTile];           // the tile in its sorted order
    __shared__ uint32_t wcnt[kOrdWaves][kOrdDigits];  // per wave and digit: running count, then start in the tile
    __shared__ uint32_t base[kOrdDigits];           // where the block's next word of digit d goes
    __shared__ uint32_t gofs[kOrdDigits];           // base[d] - the start of digit d in the tile
    __shared__ uint32_t wsum[kOrdWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t below = (1ull << lane) - 1;
    base[tid] = tid <= a.mask ? a.count[(int64_t)tid * gridDim.x + blockIdx.x] : 0;
    int64_t t0, t1;
    own_tiles(a.tiles, &t0, &t1);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t tile0 = t * kOrdTile;
        const int live = (int)(a.n - tile0 < kOrdTile ? a.n - tile0 : kOrdTile);  // words of this tile
#pragma unroll
        for (int w = 0; w < kOrdWaves; ++w) wcnt[w][tid] = 0;
        uint64_t word[kOrdRounds];
        uint32_t rank[kOrdRounds];
#pragma unroll
        for (int r = 0; r < kOrdRounds; ++r) {  // the wave's quarter, 64 consecutive words a round
            const int p = (wave * kOrdRounds + r) * 64 + lane;
            word[r] = p < live ? word_at<FIRST>(a, tile0 + p) : 0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kOrdRounds; ++r) {
            const bool valid = (wave * kOrdRounds + r) * 64 + lane < live;
            const uint32_t d = digit_of(word[r], a);
            uint64_t peers = __ballot(valid);
#pragma unroll
            for (int b = 0; b < kOrdBits; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t vote = __ballot(bit);
                peers &= bit ? vote : ~vote;
            }
            const uint32_t prev = wcnt[wave][d];  // every peer reads before the first of them writes
            const uint32_t mine = (uint32_t)__popcll(peers & below);
            rank[r] = prev + mine;
            if (valid && mine == 0) wcnt[wave][d] = prev + (uint32_t)__popcll(peers);
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        {  // thread d: the waves' counts of digit d to their starts in the tile's sorted order
            uint32_t c[kOrdWaves], total = 0;
#pragma unroll
            for (int w = 0; w < kOrdWaves; ++w) {
                c[w] = wcnt[w][tid];
                total += c[w];
            }
            const uint32_t incl = wave_incl(total);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t start = incl - total;
#pragma unroll
            for (int w = 0; w < kOrdWaves; ++w)
                if (w < wave) start += wsum[w];
            gofs[tid] = base[tid] - start;
            base[tid] += total;
#pragma unroll
            for (int w = 0; w < kOrdWaves; ++w) {
                wcnt[w][tid] = start;
                start += c[w];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kOrdRounds; ++r) {
            if ((wave * kOrdRounds + r) * 64 + lane < live) {
                const uint32_t p = wcnt[wave][digit_of(word[r], a)] + rank[r];
                if (p < (uint32_t)kOrdTile) sorted[p] = word[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kOrdPerThread; ++k) {
            const int p = k * kCoBlock + tid;
            if (p < live) {
                const uint64_t w = sorted[p];
                const uint32_t g = gofs[digit_of(w, a)] + (uint32_t)p;
                if ((int64_t)g < a.n) {  // always, when the counts are this input's
                    if constexpr (LAST) {
                        a.out[g] = (a.first + (w >> 32)) ^ kSignBit;
                        a.vout[g] = (uint32_t)w;
                    } else {
                        a.out[g] = w;
                    }
                }
            }
        }
        // the next tile's first barrier stands between these reads of gofs and its rewrite
    }
}

}  // namespace

int co_order_passes(uint64_t span) {
    int bits = 1;
    while (bits < 32 && (span - 1) >> bits) ++bits;
    return (bits + kOrdBits - 1) / kOrdBits;
}

size_t co_order_count_bytes() { return (size_t)kOrdDigits * kOrdMaxBlocks * 4; }

void co_launch_order(const OrderP& o, hipStream_t st) {
    int bits = 1;
    while (bits < 32 && (o.span - 1) >> bits) ++bits;
    const int P = co_order_passes(o.span);
    const int64_t tiles = (o.n + kOrdTile - 1) / kOrdTile;
    const dim3 grid((unsigned)(tiles < kOrdMaxBlocks ? tiles : kOrdMaxBlocks)), blk(kCoBlock);
    uint64_t* buf[2] = {o.a, o.b};
    int shift = 0;
    for (int p = 0; p < P; ++p) {
        const int width = bits / P + (p < bits % P ? 1 : 0);  // the digits spread evenly over the passes
        const bool first = p == 0, last = p == P - 1;
        Pass a;
        a.keys = o.keys;
        a.in = first ? nullptr : buf[(p - 1) & 1];
        a.out = last ? o.kout : buf[p & 1];  // the last pass reads a or b and writes neither
        a.vout = o.vout;
        a.count = o.count;
        a.flag = o.flag;
        a.n = o.n;
        a.first = o.first;
        a.span = o.span;
        a.tiles = tiles;
        a.epoch = o.epoch;
        a.shift = shift;
        a.mask = (1 << width) - 1;
        shift += width;
        if (first) hipLaunchKernelGGL((k_ord_count<true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((k_ord_count<false>), grid, blk, 0, st, a);
        hipLaunchKernelGGL(k_ord_scan, dim3(1), dim3(kScanThreads), 0, st, o.count, (int64_t)(a.mask + 1) * grid.x);
        if (first && last) hipLaunchKernelGGL((k_ord_scatter<true, true>), grid, blk, 0, st, a);
        else if (first) hipLaunchKernelGGL((k_ord_scatter<true, false>), grid, blk, 0, st, a);
        else if (last) hipLaunchKernelGGL((k_ord_scatter<false, true>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((k_ord_scatter<false, false>), grid, blk, 0, st, a);
    }
}

}  // namespace dml

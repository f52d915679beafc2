// dml_pull.hip — the two kernels of dml_group_pull and their
// diagnostic entry dml_diag_pull_kernels.
//
// The reference worker's fetch (WorkerAgent.fetch, WorkerAgent.java:74-122) intersects
// the requested keys with every server's partition and gets the answers back as one
// byte[] per server. For a key list already in HBM that is
//
//   the key partition   a stable partition of an int64 list by owner shard under
//                       KeyRange.linearSplit(world) (KeyRange.java:68-80): the keys as
//                       [owner][list order] (what each owner is asked for), per-owner
//                       counts plus the dropped count (keys outside [0, total_rows), tested
//                       as 64-bit values like dml_shard_split's), and for every list index
//                       its owner-major slot and its kept index (the list index minus the
//                       dropped keys before it: the dropped bucket of the same scan). The
//                       dml_split.hip scheme for bare keys:
//     k_pull_count      per block of kPullTile keys: LDS histogram -> blkcnt[block][owner]
//                       (integer counts: their order changes nothing)
//     k_pull_scan       per owner: exclusive scan of the block counts, and the total
//     k_pull_scatter    per block: a key's place is its block's offset + the count of its
//                       owner in the block's earlier rounds and waves + its rank among the
//                       wave's lanes of the same owner (ballots, no atomics)
//
//   k_pull_unsplit      request-order mode: the owner-major receive buffer permuted into
//                       dev_out, record j of the output = record perm[j] of the input.
//                       Output-stationary like k_fetch_vec (dml_fetch.hip): one thread per
//                       16-byte line of the output ADDRESS, one division per line; a line
//                       inside one record is one 4-byte-aligned 16-byte load and one
//                       non-temporal 16-byte store; single dwords only at the stream's first
//                       and last line. Bytes move as uint32: no float instruction sees them.
#include <algorithm>
#include <string>
#include <vector>

#include "dml_device.h"
#include "dml_host.h"

namespace dml {

namespace {

constexpr int kPullBlock = 256;
constexpr int kPullRounds = 4;  // keys per thread; round u takes keys base + u x 256 + thread
constexpr int kPullTile = kPullBlock * kPullRounds;
constexpr int kPullWaves = kPullBlock / 64;
constexpr int kMaxWorld = DML_PULL_MAX_WORLD;  // the LDS tables below hold one entry per owner plus the dropped bucket
constexpr int kUnsplitBlock = 256;             // lines (threads) per block of k_pull_unsplit
static_assert(DML_PULL_WAVE_BYTES == 64 * 16 && DML_PULL_BLOCK_BYTES == kUnsplitBlock * 16,
              "the exported tile sizes are k_pull_unsplit's");

__device__ inline int pull_owner(int64_t key, int64_t total_rows, int64_t step, int world) {
    if (key < 0 || key >= total_rows) return world;  // dropped
    const int64_t d = key / step;
    return d < world ? (int)d : world;
}

__global__ __launch_bounds__(kPullBlock) void k_pull_count(const int64_t* __restrict__ keys, int64_t n,
                                                          int64_t total_rows, int64_t step, int world,
                                                          int32_t* __restrict__ blkcnt) {
    __shared__ int32_t h[kMaxWorld + 1];
    if (threadIdx.x <= world) h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPullTile + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kPullRounds; ++u) {
        const int64_t i = base + u * kPullBlock;
        if (i < n) atomicAdd(&h[pull_owner(keys[i], total_rows, step, world)], 1);
    }
    __syncthreads();
    if (threadIdx.x <= world) blkcnt[(int64_t)blockIdx.x * (world + 1) + threadIdx.x] = h[threadIdx.x];
}

// grid (world + 1): blkoff[blk][d] = sum of blkcnt[0..blk)[d]; tot[d] = the sum over all blocks.
__global__ __launch_bounds__(256) void k_pull_scan(const int32_t* __restrict__ blkcnt, int64_t nblk, int world,
                                                  int64_t* __restrict__ blkoff, int64_t* __restrict__ tot) {
    __shared__ int64_t part[256];
    const int d = blockIdx.x, W1 = world + 1;
    const int64_t per = (nblk + 255) / 256;
    const int64_t lo = threadIdx.x * per < nblk ? threadIdx.x * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += blkcnt[i * W1 + d];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {  // 256 partial sums: a serial scan is cheaper than a tree here
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
        tot[d] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        blkoff[i * W1 + d] = run;
        run += blkcnt[i * W1 + d];
    }
}

// Every output but out_keys may be null (the group needs perm in request-order mode only).
__global__ __launch_bounds__(kPullBlock) void k_pull_scatter(const int64_t* __restrict__ keys, int64_t n,
                                                            int64_t total_rows, int64_t step, int world,
                                                            const int64_t* __restrict__ blkoff,
                                                            const int64_t* __restrict__ tot,
                                                            int64_t* __restrict__ out_keys, int64_t* __restrict__ slot,
                                                            int64_t* __restrict__ kept, int64_t* __restrict__ perm) {
    __shared__ int64_t start[kMaxWorld + 1];            // owner d's first slot for this block's next round
    __shared__ int32_t wcnt[kPullRounds][kPullWaves][kMaxWorld + 1];  // keys of owner d in wave w of round u
    const int W1 = world + 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    if (threadIdx.x <= world) {
        int64_t b = 0;  // owner-major: the owners before d come first; the dropped bucket counts from 0
        for (int q = 0; q < (int)threadIdx.x && (int)threadIdx.x < world; ++q) b += tot[q];
        start[threadIdx.x] = b + blkoff[(int64_t)blockIdx.x * W1 + threadIdx.x];
    }
    for (int t = threadIdx.x; t < kPullRounds * kPullWaves * (kMaxWorld + 1); t += kPullBlock) (&wcnt[0][0][0])[t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kPullTile + threadIdx.x;
    for (int u = 0; u < kPullRounds; ++u) {
        const int64_t i = base + u * kPullBlock;
        const bool live = i < n;
        const int64_t key = live ? keys[i] : 0;
        const int d = live ? pull_owner(key, total_rows, step, world) : -1;
        // rank among the wave's lanes of the same owner: peel one owner per turn (at most world + 1)
        int rank = 0;
        unsigned long long rest = __ballot(live);
        while (rest) {
            const int lead = __ffsll((long long)rest) - 1;
            const int dl = __shfl(d, lead);
            const unsigned long long m = __ballot(d == dl);
            if (d == dl) {
                rank = __popcll(m & below);
                if (rank == 0) wcnt[u][wave][d] = __popcll(m);
            }
            rest &= ~m;
        }
        const int drop_below = __popcll(__ballot(live && d == world) & below);
        __syncthreads();  // also: start[] holds the rounds before this one
        if (live) {
            int before = 0, drops = 0;  // in the earlier waves of this round
            for (int w = 0; w < wave; ++w) {
                before += wcnt[u][w][d];
                drops += wcnt[u][w][world];
            }
            if (d < world) {
                const int64_t p = start[d] + before + rank;
                const int64_t j = i - (start[world] + drops + drop_below);
                out_keys[p] = key;
                if (slot) slot[i] = p;
                if (kept) kept[i] = j;
                if (perm) perm[j] = p;
            } else {
                if (slot) slot[i] = -1;
                if (kept) kept[i] = -1;
            }
        }
        __syncthreads();
        if (threadIdx.x <= world) {
            int c = 0;
            for (int w = 0; w < kPullWaves; ++w) c += wcnt[u][w][threadIdx.x];
            start[threadIdx.x] += c;
        }
    }
}

struct UnsplitP {
    const uint32_t* src;  // the owner-major records, as dwords
    const int64_t* perm;  // output record -> input record
    uint8_t* line0;       // dst rounded down to 16 bytes
    int64_t ndw;          // dwords of the stream
    int32_t recdw, lead;
};

__device__ inline void stg32_nt(void* p, uint32_t v) { __builtin_nontemporal_store(v, (DML_GLOBAL uint32_t*)p); }

// One block: kUnsplitBlock lines = DML_PULL_BLOCK_BYTES of output; one wave instruction's 64 lines are
// contiguous (DML_PULL_WAVE_BYTES).
template <bool VLOAD>
__global__ __launch_bounds__(kUnsplitBlock) void k_pull_unsplit(const UnsplitP a, int64_t nline) {
    const int64_t v = (int64_t)blockIdx.x * kUnsplitBlock + threadIdx.x;
    if (v >= nline) return;
    const int64_t d0 = 4 * v - a.lead;  // stream dword of the line's first slot (< 0 only on line 0)
    const int64_t lo = d0 < 0 ? 0 : d0;
    const int64_t hi = d0 + 4 < a.ndw ? d0 + 4 : a.ndw;
    if (lo >= hi) return;
    int64_t j;
    if (a.ndw <= 0xFFFFFFFFll) j = (int64_t)((uint32_t)lo / (uint32_t)a.recdw);
    else j = lo / a.recdw;
    int32_t w = (int32_t)(lo - j * a.recdw);  // dword inside record j
    const uint32_t* rec = a.src + a.perm[j] * a.recdw;
    uint8_t* o = a.line0 + 16 * v;
    if (VLOAD && hi - lo == 4 && w + 4 <= a.recdw) {
        stg16_nt(o, ldg16((const uint8_t*)(rec + w)));
        return;
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
            rec = a.src + a.perm[j] * a.recdw;
        }
        val[e] = ldg32((const uint8_t*)(rec + w));
        mask |= 1u << e;
        ++w;
    }
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

}  // namespace

int64_t pull_partition_blocks(int64_t n) { return (n + kPullTile - 1) / kPullTile; }

// Workspace of one partition: blkcnt int32 [nblk][world + 1], then (256-byte aligned)
// blkoff int64 [nblk][world + 1].
size_t pull_partition_ws_bytes(int64_t n, int world) {
    const size_t e = (size_t)pull_partition_blocks(n) * (size_t)(world + 1);
    return ((e * 4 + 255) & ~(size_t)255) + e * 8;
}

// tot: device int64 [world + 1], the per-owner counts and the dropped count. n > 0.
hipError_t launch_pull_partition(const int64_t* keys, int64_t n, int64_t total_rows, int64_t step, int world,
                                 uint8_t* ws, int64_t* out_keys, int64_t* slot, int64_t* kept, int64_t* perm,
                                 int64_t* tot, hipStream_t st) {
    if (world <= 0 || world > kMaxWorld) return hipErrorInvalidValue;  // the kernels' LDS tables
    const int64_t nblk = pull_partition_blocks(n);
    int32_t* blkcnt = (int32_t*)ws;
    int64_t* blkoff = (int64_t*)(ws + (((size_t)nblk * (size_t)(world + 1) * 4 + 255) & ~(size_t)255));
    hipLaunchKernelGGL(k_pull_count, dim3((unsigned)nblk), dim3(kPullBlock), 0, st, keys, n, total_rows, step, world,
                       blkcnt);
    hipLaunchKernelGGL(k_pull_scan, dim3((unsigned)(world + 1)), dim3(256), 0, st, blkcnt, nblk, world, blkoff, tot);
    hipLaunchKernelGGL(k_pull_scatter, dim3((unsigned)nblk), dim3(kPullBlock), 0, st, keys, n, total_rows, step, world,
                       blkoff, tot, out_keys, slot, kept, perm);
    return hipGetLastError();
}

// Records of at least this many dwords take the 16-byte loads; shorter ones gather every
// dword singly. DESIGN.md §4.11: records of 201 and 257 dwords run 1-3 % faster gathered,
// records of 401 and 1001 dwords 5 % and 5-15 % faster with the loads; the threshold sits
// between the two measured neighbours.
constexpr int32_t kPullVloadMinDw = 320;

// dst record j = src record perm[j], nrec records of rec_bytes (a multiple of 4); src and dst
// are 4-byte aligned. variant: 0 = by record length, 1 = dword gathers, 2 = 16-byte loads.
hipError_t launch_pull_unsplit(const void* src, const int64_t* perm, int64_t nrec, int64_t rec_bytes, void* dst,
                               int variant, hipStream_t st) {
    if (nrec <= 0) return hipSuccess;
    UnsplitP a;
    a.src = (const uint32_t*)src;
    a.perm = perm;
    a.lead = (int32_t)(((uintptr_t)dst & 15) >> 2);
    a.line0 = (uint8_t*)dst - 4 * a.lead;
    a.recdw = (int32_t)(rec_bytes / 4);
    a.ndw = nrec * a.recdw;
    const int64_t nline = (a.ndw + a.lead + 3) / 4;
    const bool vload = variant == 2 || (variant == 0 && a.recdw >= kPullVloadMinDw);
    const dim3 grid((unsigned)((nline + kUnsplitBlock - 1) / kUnsplitBlock));
    if (vload) hipLaunchKernelGGL(k_pull_unsplit<true>, grid, dim3(kUnsplitBlock), 0, st, a, nline);
    else hipLaunchKernelGGL(k_pull_unsplit<false>, grid, dim3(kUnsplitBlock), 0, st, a, nline);
    return hipGetLastError();
}

}  // namespace dml

using namespace dml;

extern "C" int dml_diag_pull_kernels(const int64_t* dev_keys, int64_t nkeys, int64_t total_rows, int32_t world,
                                     int64_t* dev_part_keys, int64_t* dev_slot, int64_t* dev_kept, int64_t* counts,
                                     const void* dev_src, void* dev_dst, int64_t rec_bytes, int32_t variant,
                                     void* stream, float* ms_partition, float* ms_unsplit) {
    if (nkeys < 0 || total_rows <= 0 || world <= 0 || world > kMaxWorld || !counts ||
        (nkeys > 0 && (!dev_keys || !dev_part_keys)) || variant < 0 || variant > 2)
        return set_error(DML_E_INVALID_ARG, "bad pull kernel arguments (world <= 64)");
    if (((uintptr_t)dev_keys | (uintptr_t)dev_part_keys | (uintptr_t)dev_slot | (uintptr_t)dev_kept) & 7u)
        return set_error(DML_E_INVALID_ARG, "key and index buffers are 8-byte aligned");
    const bool unsplit = dev_src && dev_dst;
    if (unsplit && (rec_bytes < 8 || rec_bytes % 4 || rec_bytes / 4 > 0x7FFFFFFF ||
                    (((uintptr_t)dev_src | (uintptr_t)dev_dst) & 3u)))
        return set_error(DML_E_INVALID_ARG, "records are whole dwords at 4-byte aligned addresses");
    if (ms_partition) *ms_partition = 0.f;
    if (ms_unsplit) *ms_unsplit = 0.f;
    for (int d = 0; d <= world; ++d) counts[d] = 0;
    if (nkeys == 0) return DML_OK;
    std::vector<int64_t> f((size_t)world), l((size_t)world);
    if (int rc = dml_linear_split(0, total_rows - 1, world, f.data(), l.data())) return rc;
    const int64_t step = l[0] - f[0] + 1;
    hipStream_t st = (hipStream_t)stream;
    const size_t wsb = (pull_partition_ws_bytes(nkeys, world) + 255) & ~(size_t)255;
    const size_t totb = 1024;  // world + 1 <= 65 int64
    uint8_t* ws = nullptr;
    HIPCHK(hipMalloc((void**)&ws, wsb + totb + (size_t)nkeys * 8));
    int64_t* tot = (int64_t*)(ws + wsb);
    int64_t* perm = (int64_t*)(ws + wsb + totb);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (hipEvent_t& x : ev)
        if (e == hipSuccess) e = hipEventCreate(&x);
    if (e == hipSuccess) e = hipEventRecord(ev[0], st);
    if (e == hipSuccess)
        e = launch_pull_partition(dev_keys, nkeys, total_rows, step, world, ws, dev_part_keys, dev_slot, dev_kept, perm,
                                  tot, st);
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
    if (e == hipSuccess) e = hipMemcpyAsync(counts, tot, sizeof(int64_t) * (size_t)(world + 1), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    int64_t nrec = 0;
    for (int d = 0; d < world; ++d) nrec += counts[d];
    if (e == hipSuccess && unsplit) {
        e = hipEventRecord(ev[2], st);
        if (e == hipSuccess) e = launch_pull_unsplit(dev_src, perm, nrec, rec_bytes, dev_dst, variant, st);
        if (e == hipSuccess) e = hipEventRecord(ev[3], st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && ms_unsplit) e = hipEventElapsedTime(ms_unsplit, ev[2], ev[3]);
    }
    if (e == hipSuccess && ms_partition) e = hipEventElapsedTime(ms_partition, ev[0], ev[1]);
    for (hipEvent_t x : ev)
        if (x) (void)hipEventDestroy(x);
    (void)hipFree(ws);
    if (e != hipSuccess) return set_error(DML_E_HIP, std::string("pull kernels: ") + hipGetErrorString(e));
    return DML_OK;
}

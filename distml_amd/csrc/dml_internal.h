// dml_internal.h — types shared by the HIP kernel files and the C-ABI host
// implementation (dml_store*.hip, dml_prereduce.hip), and the kernels' launchers.
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

struct dml_store;

namespace dml {

// One ordered batch chunk holds at most this many pushes (the slot table is
// [rows][kMaxW] int32); longer batches run as consecutive chunks, in order.
constexpr int kMaxW = 64;
// Row stride of a chunk's slot table: its push count rounded up to 8 (scalar slot
// loads read 8 entries at a time). [rows][stride] instead of [rows][64]: an
// 8-push chunk of config 4's 1.25 M rows indexes into 40 MB (stays in the 256 MB
// MALL) instead of 320 MB. Allocations stay rows x kMaxW.
__host__ __device__ inline int slot_stride(int nb) { return (nb + 7) & ~7; }

// Position of a byte in the batch, in reference processing order:
// bucket-major, then byte offset inside the bucket (the order in which
// handlePush's while-loop reads bytes, FloatMatrixStore.java:202-207).
__host__ __device__ inline uint64_t pos_of(uint64_t bucket, uint64_t off) { return (bucket << 40) | off; }
constexpr uint64_t kNoPos = ~0ull;
constexpr uint64_t kOffMask = (1ull << 40) - 1;

// Per-batch control block. Lives at the head of the workspace
// [Ctrl | slot rows x kMaxW int32 | rowflag rows x uint32]: one hipMemsetAsync(0xFF)
// resets Ctrl and the slot table (-1 = no record); rowflag is zeroed separately.
struct Ctrl {
    unsigned long long cutoff;   // first key-out-of-shard position (exclusive apply limit)
    unsigned long long neg_pos;  // first add that left an int32 counter negative
    unsigned long long ident;    // speculative chunk: bit b = push b verified in the reduce (identity: record r is row r; or slot reuse)
    unsigned int no_dup;         // 0xFFFFFFFF = no row repeated inside one push; 0 = repeat seen
    unsigned int spec_ok;        // speculative chunk: 0xFFFFFFFF = every identity record verified; 0 = not
    // Slot-table column of push b (0xFF, the reset value: column b). k_index writes a
    // push's records there and the reduce reads them from there. In a speculative
    // chunk a push whose `ident` bit is set takes slot = row when its column is 0xFF
    // (identity) and otherwise reads the kept column k_ident_check matched it to
    // (slot reuse, whatever position the push arrived at).
    unsigned char col[kMaxW];
};
static_assert(sizeof(Ctrl) == 96, "Ctrl layout (a multiple of 32 B: the slot table after it stays aligned)");
__host__ __device__ inline int ctrl_col(const Ctrl* c, int b) {
    const unsigned v = c->col[b];
    return v == 0xFFu ? b : (int)v;
}
// A speculative chunk's push b verified as identity (record r holds row r).
__host__ __device__ inline bool ctrl_identity(const Ctrl* c, unsigned long long ident, int b) {
    return ((ident >> b) & 1ull) && c->col[b] == 0xFFu;
}

// Bucket table passed by value as a kernel argument (scalar-loaded).
struct Batch {
    const uint8_t* base[kMaxW];
    int64_t len[kMaxW];
    int64_t nrec[kMaxW];  // records whose key is complete (a truncated tail record included)
    int32_t bidx[kMaxW];  // global push index of each column (positions use it; columns ascend)
    const Ctrl* prev;     // control block of the chunk enqueued just before (pipelining), or null
    // Identity speculation (full-range chunks of plain sums): pushes
    // whose sampled keys say "record r holds row r" skip the key index; the reduce
    // takes slot = row for them and verifies every such record's key, reading the
    // input shard at `src` and writing the output buffer (the host keeps the input
    // until the chunk retires, so a failed verification re-runs it exactly).
    const void* src;      // input shard (null: in place)
    int64_t first;        // key of row 0 (KeyRange first), for the verification
    int32_t spec;         // 1: speculative chunk
    // Slot reuse (speculative chunks): bit c = column c of the workspace's slot table
    // still holds the permutation a push of the workspace's previous chunk listed
    // (verified there). A push whose sampled keys match one of these columns, at any
    // position, skips the key index (k_ident_check sets Ctrl::col); the reduce reads
    // its slots from that column and verifies every record's key.
    uint64_t kept_cols;
    // 1: such a chunk (its table may hold kept columns, so a stale entry is no
    // repeat): the key index does not look for repeated rows, and the reduce
    // verifies the record of every row of every push instead (all pushes are
    // full-range, so a repeat leaves another row without its record).
    int32_t keeps;
    // 1: the Ctrl::ident pushes were verified record by record before this launch
    // (k_ident_full; the sharded pre-reduce, whose partial the reduce-scatter takes
    // before a speculative verdict could be read): the reduce takes slot = row for
    // them and verifies nothing.
    int32_t ident_ok;
    // Rows any push of the chunk lists (byte per row, written by the key index; null:
    // not tracked). Sparse-row chunks of k_reduce_rows (LDA's 65 536-row pushes into a
    // 1 M-row table, config 5) leave ~11 % of the rows untouched: their shard rows are
    // then neither read nor written.
    const uint8_t* listed;
};

// A chunk whose predecessor ended abnormally (error, rows to replay, or a failed
// identity speculation) must not run ahead of the host's fix-up: its kernels
// turn into no-ops and the host relaunches (replay) or drops (error) it.
// Every field is read and the tests combined without short-circuit: in a kernel the
// four loads issue together (one wait) instead of as a chain of dependent round trips
// ahead of the block's first data load.
__host__ __device__ inline bool ctrl_abnormal(const Ctrl* c) {
    const unsigned long long cut = c->cutoff, neg = c->neg_pos;
    const unsigned int nd = c->no_dup, ok = c->spec_ok;
    return (cut != kNoPos) | (neg != kNoPos) | (nd == 0u) | (ok == 0u);
}

// Per-block AdaGrad candidate: the largest final delta of an element whose
// delta rose in this batch, and the position where it last rose.
struct DeltaCand {
    float value;
    int32_t valid;
    unsigned long long pos;
};
// Running AdaGrad maxDelta state (FloatMatrixStoreAdaGrad.java:27-29), device
// resident, plus the chunk's best candidate while it waits for the rows a push
// repeats (replayed in layers): the chunk's candidates are finalized once, so a
// tie between a repeated and a non-repeated row goes to the earlier position.
struct MaxDelta {
    float value;
    int32_t row;
    int32_t col;
    int32_t pad;
    DeltaCand pend;
};
static_assert(sizeof(MaxDelta) == 32, "MaxDelta layout (DML_MAXDELTA_RECORD_BYTES: a chained AdaGrad slice carries one)");
// k_maxdelta finalize modes
enum MdMode : int {
    kMdApply = 0,          // merge with the pending candidate, apply (strict >), clear it
    kMdDefer = 1,          // merge into the pending candidate only
    kMdDeferIfRepeat = 2,  // kMdDefer when the chunk's index saw a repeated row (ctrl->no_dup == 0)
};

// Optional row map of a reduce launch (multi-GPU pre-reduce pieces): task row t
// reduces shard row  (t / block) * stride + off + t % block  (block == 0: row = t)
// and writes it to out + t*cols (out == null: in place). Rows >= rows_total are
// padding of linearSplit's short last shard: written as zeros.
// kChain launches: the accumulator of task row t starts from base + t*cols (the
// slice as it arrived; out == base works, every element is read and written by one
// lane), and padding rows are copied from base.
struct RowMap {
    int64_t block = 0, stride = 0, off = 0;
    int64_t rows_total = 0;
    void* out = nullptr;
    const void* base = nullptr;
    // kChainCheckI32: the slice's travelling verdict record (ChainI32Rec); closed = copy
    const void* rec = nullptr;
    // model row of task row t (rows <= INT32_MAX, a Java array: 32-bit division)
    __host__ __device__ inline int64_t row(int64_t t) const {
        if (!block) return t;
        const uint32_t q = (uint32_t)t / (uint32_t)block;
        return (int64_t)q * stride + off + (int64_t)((uint32_t)t - q * (uint32_t)block);
    }
};

struct AdaArgs {
    float* alpha;
    float* delta;
    DeltaCand* cand;      // one per reduce block
    float initial_alpha, min_alpha, factor;
};

enum ReduceMode : int {
    kAdd = 0,          // f32 / f64 / i32-without-check
    kAddCheckI32 = 1,  // IntMatrixStore dense: negativity check after each add
    kAdaGrad = 2,      // FloatMatrixStoreAdaGrad dense
    kRollbackI32 = 3,  // undo adds after the first negative (exact mod 2^32)
    kPreReduce = 4,    // multi-GPU pre-reduce: acc starts at 0, every row written
    // Chained reduce-scatter step (f32 / f64): acc starts at RowMap::base, the pushes'
    // records are added in push order as kAdd adds them, every row is written to
    // RowMap::out; a row no push lists is copied bit for bit (no add of +0.0, which
    // would turn -0.0 into +0.0). A handle whose index met a key outside the matrix
    // or a repeated row adds nothing: every row is copied.
    kChain = 5,
    // Chained reduce-scatter step of an int32 matrix: kChain's row rules with
    // kAddCheckI32's check after every add. The first position (push << 40 | byte
    // offset) that left a counter negative goes to Ctrl::neg_pos by atomicMin; every
    // add is made (kRollbackI32 through the piece's row map undoes the later ones once
    // the whole slice has been summed). A slice whose record (RowMap::rec) arrived
    // closed is copied bit for bit, like one whose handle's index failed.
    kChainCheckI32 = 6,
};
// The verdict record an int32 slice carries round the ring, at the head of its first
// sub-chunk's message (DML_CHAIN_I32_RECORD_BYTES; 8-byte aligned). Open: pos == kNoPos.
struct ChainI32Rec {
    unsigned long long pos;  // (push << 40) | byte offset of the failing add in the closing rank's push
    long long key;           // IllegalStateException(key, col), IntMatrixStore.java:174-176
    int32_t col;
    int32_t step;            // ring step at which the slice closed
    unsigned long long pad;
};
static_assert(sizeof(ChainI32Rec) == 32, "ChainI32Rec layout (DML_CHAIN_I32_RECORD_BYTES)");
// kChain: the index's verdict, read by every wave (nothing of a failed call is added)
__host__ __device__ inline bool ctrl_index_failed(const Ctrl* c) {
    const unsigned long long cut = c->cutoff;
    const unsigned int nd = c->no_dup;
    return (cut != kNoPos) | (nd == 0u);
}

enum VType : int { kI32 = 0, kF32 = 1, kF64 = 3 };

// Optional start/stop events carried in the dispatch packet (hipExtLaunchKernel):
// kernel timing and cross-stream dependencies without extra marker packets.
struct LaunchEv {
    hipEvent_t start = nullptr;
    hipEvent_t stop = nullptr;
};

// ---- launchers, grouped by the file that holds the kernels ----
// ---- dense push path (dml_kernels.hip) ----
hipError_t launch_index(const Batch& bt, int nb, int64_t max_nrec, int64_t stride, int K,
                        int64_t first, int64_t rows, int32_t* slot, uint32_t* rowflag, Ctrl* ctrl,
                        uint64_t tail_cut, hipStream_t st);
// Identity speculation: clears ctrl->ident bit b unless push b is full-range and
// every sampled record r of it has row_index(key) == r (Ctrl reset to all ones).
hipError_t launch_ident_check(const Batch& bt, int nb, int64_t stride, int K, int64_t first, int64_t rows,
                              const int32_t* slot, Ctrl* ctrl, hipStream_t st);
// After k_ident_check of a chunk offered kept columns: gives every push that is
// neither identity nor matched a slot-table column no matched push reads
// (Ctrl::col), so its key index does not overwrite a reused permutation.
hipError_t launch_assign_cols(Ctrl* ctrl, int nb, hipStream_t st);
// Complete identity check (Ctrl::ident reset to all ones, or as k_ident_check left
// it): clears ctrl->ident bit b unless every record r of push b has row_index(key) == r.
hipError_t launch_ident_full(const Batch& bt, int nb, int64_t max_nrec, int64_t stride, int K, int64_t first,
                             int64_t rows, Ctrl* ctrl, hipStream_t st);
hipError_t launch_reduce(int vtype, int mode, void* shard, int64_t rows, int32_t cols, const Batch& bt,
                         int nb, int64_t stride, int K, const int32_t* slot, const uint32_t* rowflag, Ctrl* ctrl,
                         uint64_t tail_cut, const AdaArgs& ada, hipStream_t st, int64_t* nblocks_out,
                         LaunchEv ev = {}, RowMap rm = {});
hipError_t launch_rollback_i32(int32_t* shard, int64_t rows, int32_t cols, const Batch& bt, int nb,
                               int64_t stride, int K, const int32_t* slot, const uint32_t* rowflag, Ctrl* ctrl,
                               uint64_t tail_cut, hipStream_t st, RowMap rm = {});
// `cand` holds n candidates plus kMdParts entries of scratch after them.
constexpr int kMdParts = 256;
hipError_t launch_maxdelta_finalize(DeltaCand* cand, int64_t n, MaxDelta* md, const Batch& bt, int nb,
                                    int64_t stride, int K, int V, hipStream_t st, int mode = kMdApply,
                                    const Ctrl* ctrl = nullptr);

// ---- chained reduce-scatter steps and commits (dml_chain.hip) ----
// After the chained int32 step's rollback (one wave): a set Ctrl::neg_pos closes an open
// record (pos, the key read from the push at pos, col, ring step); the word is reset.
hipError_t launch_chain_i32_verdict(const Batch& bt, int nb, int64_t stride, int K, Ctrl* ctrl, ChainI32Rec* rec,
                                    int32_t step, hipStream_t st, LaunchEv ev = {});
// The owner's commit: the home record closes the store's open record (sticky).
hipError_t launch_chain_i32_merge(ChainI32Rec* store_rec, const ChainI32Rec* home, hipStream_t st);
// Chained reduce-scatter step of an AdaGrad matrix: the planes beside
// RowMap::base / RowMap::out (data). Marks: one uint32 per task row, non-zero = some
// rank's accepted push listed the row in this call; base_marks == null reads as all
// clear (ring step 0).
struct ChainAda {
    const float* base_delta;
    float* out_delta;
    const uint32_t* base_marks;
    uint32_t* out_marks;
    DeltaCand* cand;  // one per block (chain_ada_blocks)
};
// ident: k_chain_ada_ident (every push confirmed identity by k_ident_full, rows of
// whole 16-B vectors); otherwise k_chain_ada_rows over the slot table.
int64_t chain_ada_blocks(bool ident, int64_t ntask, int32_t cols);
hipError_t launch_chain_ada(bool ident, int64_t ntask, int32_t cols, const Batch& bt, int nb, int64_t stride, int K,
                            int32_t* slot, const Ctrl* ctrl, RowMap rm, const ChainAda& ca, hipStream_t st,
                            int64_t* ncand_out, LaunchEv ev);
// The owner's commit of the slice that came home: data, delta, alpha where marked and
// delta > 1 (ada's parameters), and the running maxDelta = *rec.
hipError_t launch_chain_ada_commit(float* data, float* delta, float* alpha, MaxDelta* md, const float* sdata,
                                   const float* sdelta, const uint32_t* marks, const MaxDelta* rec, int64_t rows,
                                   int32_t cols, const AdaArgs& ada, hipStream_t st);

// ---- two-moment AdaGrad (dml_moments.hip; sharded path) ----
// Per-rank [row][Σu | Σu²] pre-reduce pieces (flat shapes: cols % 4 == 0, rows under
// 4 KiB), and the owner apply of the reduce-scattered moments (+ maxDelta finalize;
// ada.cand holds kMomentBlocks entries).
constexpr int kMomentBlocks = 2048;
hipError_t launch_moments(int64_t ntask, int32_t cols, const Batch& bt, int nb, int64_t stride, int K, int32_t* slot,
                          const Ctrl* ctrl, RowMap rm, hipStream_t st, LaunchEv ev);
hipError_t launch_ada_moments(float* shard, const float* src, int64_t rows, int32_t cols, const AdaArgs& ada,
                              MaxDelta* md, int64_t first, hipStream_t st, LaunchEv ev);

// ---- a store's other operations (dml_ops.hip) ----
hipError_t launch_array_rollback_i32(int32_t* shard, int64_t rows, const uint8_t* base, int64_t nrec,
                                     int b_global, int64_t stride, int K, int64_t first, Ctrl* ctrl,
                                     uint64_t tail_cut, hipStream_t st);
hipError_t launch_key_rows(const uint8_t* base, int64_t nrec, int64_t stride, int K, int64_t first, int64_t rows,
                           int32_t* out, hipStream_t st);
hipError_t launch_rand(int vtype, void* p, int64_t rows, int32_t cols, uint64_t s0, hipStream_t st);
hipError_t launch_bswap(int V, const void* src, void* dst, int64_t n, hipStream_t st);
hipError_t launch_fill(int vtype, void* p, int64_t n, double v, hipStream_t st);
hipError_t launch_fill_f32(float* p, int64_t n, float v, hipStream_t st);
hipError_t launch_apply_dense(int vtype, void* shard, const void* src, int64_t n, hipStream_t st);
hipError_t launch_apply_dense_i32chk(int32_t* shard, const int32_t* src, int64_t n, unsigned long long* neg,
                                     hipStream_t st);
hipError_t launch_fetch(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                        int64_t key_lo, int64_t n, int64_t first, uint8_t* out, int64_t rec, int K, int value_slot,
                        hipStream_t st);
// k_fetch with the device key check of dml_store_fetch_device's list form (knob 1).
hipError_t launch_fetch_checked(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                                int64_t n, int64_t first, int64_t last, uint8_t* out, int64_t rec, int K,
                                int value_slot, unsigned long long* bad, hipStream_t st);

// ---- vectorised fetch (dml_fetch.hip) ----
// k_fetch_vec: the same records as one stream of whole 16-byte stores.
// `variant` (diagnostic, bits kFetchVar*) picks the launch shapes DESIGN.md §4.10 compares.
constexpr int kFetchVarLoadMask = 3;  // 0: by record length, 1: every dword singly, 2: 16-byte shard loads
constexpr int kFetchVarGather = 1, kFetchVarVload = 2;
constexpr int kFetchVarXcd = 4;       // blocks renumbered by xcd_block() instead of dispatch order
constexpr int kFetchVarU1 = 8;        // one vector per thread (4-KiB blocks) ...
constexpr int kFetchVarU4 = 16;       // ... or four (16-KiB blocks); neither: the shipped choice
constexpr int kFetchVariants = 24;
struct FetchVerdict {                // first key outside the shard of the list fetches so far
    unsigned long long idx;          // its list index, kNoPos: none
    int64_t key;
};
hipError_t launch_fetch_vec(int vtype, const void* shard, const float* alpha, int32_t cols, const int64_t* keys,
                            int64_t key_lo, int64_t n, int64_t first, int64_t last, uint8_t* out, int64_t rec, int K,
                            int value_slot, unsigned long long* bad, int variant, hipStream_t st);
// Behind a list fetch: *bad (this fetch's lowest bad index) into the sticky verdict, *bad reset.
hipError_t launch_fetch_verdict(unsigned long long* bad, const int64_t* keys, FetchVerdict* v, hipStream_t st);

// ---- diagnostics: synthetic data, streaming ceilings, floors (dml_diag.hip) ----
hipError_t launch_synth_fill(int vtype, void* p, int64_t n, uint64_t s0, hipStream_t st);
hipError_t launch_stream(bool copy, void* dst, const void* src, int64_t n16, hipStream_t st, LaunchEv ev);
hipError_t launch_rmw_floor(float* a, const uint32_t* idx, const float* v, int64_t n, hipStream_t st, LaunchEv ev);
hipError_t launch_dense_floor(const float* data, float* out, float* delta, const Batch& bt, int nb, int64_t stride,
                              int K, int32_t cols, int64_t elems, hipStream_t st, LaunchEv ev);
hipError_t launch_gather_floor(int32_t* shard, int32_t cols, const int32_t* trow, const int32_t* tptr,
                               const uint64_t* addr, int64_t ntouched, hipStream_t st, LaunchEv ev);
// One rank's ring reduce-scatter footprint: one kernel of `channels` blocks.
hipError_t launch_ring_rs(int vtype, const void* part, void* recv, void* land, int64_t chunk_bytes, int world,
                          int rank, int channels, hipStream_t st);
hipError_t launch_synth_dense(uint8_t* out, int K, int vtype, int64_t first, int64_t shard_rows, int64_t nrec,
                              int32_t cols, uint64_t s0, uint64_t pa, uint64_t pc, hipStream_t st);
hipError_t launch_synth_sparse(uint8_t* out, int K, int vtype, int value_stride, int64_t first,
                               int64_t key_space, int64_t nrec, uint64_t s0, uint64_t pa, uint64_t pc,
                               hipStream_t st);
// ---- ordered sparse scatter-add (dml_sparse.hip), float / double array stores ----
constexpr int kSpTile = 4096;      // records per partition tile (256 threads x 16)
constexpr int kSpLeafCap = 2048;   // records one leaf orders in LDS
constexpr uint32_t kSpSkip = 0xFFFFFFFFu;  // sequence of a record at or past the cutoff (never applied)
constexpr int kSpBigCap = 4096;    // records a big leaf orders in LDS (one-level partition)
constexpr int kSpBigBins = 16384;  // big leaves per chunk, at most (the one-level pass's LDS histogram)
constexpr int kSpSlices = 8;       // regions per big leaf: slice x holds the pushes p with p % 8 == x
// Shape of one chunk's partition (host-computed, passed by value).
struct SpPlan {
    int64_t tile_base[kMaxW + 1];  // first level-1 tile of push b (prefix of ceil(nrec / kSpTile))
    int64_t rec_base[kMaxW + 1];   // first sequence number of push b (prefix of nrec)
    int64_t nrec, ntiles1, nleaves, max_tiles2;
    int nb, SL, D2, nbins1;        // leaf = row >> SL; 2^D2 leaves per level-1 bin
    // single-pass partition (no count passes): fixed-capacity bins (cap1 records
    // per level-1 bin, cap2 per leaf) filled through atomic cursors; an overflow
    // falls back to the counted partition before the leaf runs
    int64_t cap1, cap2, tiles2_per_bin;
    int fast;                      // the leaf reads the fixed-capacity layout
    // compact records (fp32, single-pass, no cutoff): one 8-B word per record,
    // row within its level-1 bin << 38 | chunk push << 32 | value bits; the push
    // index orders a row's adds (a push listing a row twice sends its leaf to the
    // exact replay, which re-partitions with full sequence numbers)
    int compact;
    uint32_t seq_cut;              // records with sequence >= seq_cut are at / past the cutoff
    // one-level partition (compact fp32, pushes balanced over the 8 slices): "big
    // leaves" of 2^BL rows, one region of capS records per (big leaf, slice), filled
    // by the slice's tiles (pushes p % 8 == x, run by the blocks of XCD x); the leaf
    // kernel orders a big leaf's records in LDS, so there is no second pass
    int big, BL;
    int64_t nbig, capS, tiles_per_slice;
    int64_t sbase[kMaxW];          // tiles of the earlier pushes of push b's slice
};
constexpr int kSpCompactRowBits = 26;  // SL + D2 limit of the compact word
// Pinned status of a single-pass partition, read by the host before the leaf launch.
struct SpStat {
    unsigned int overflow;         // a bin or leaf exceeded its capacity
    unsigned int pad;
    unsigned long long cutoff;     // Ctrl::cutoff after the partition (first key outside the shard)
};
// Device-side results of level 1 (bin bounds, level-2 tile table).
struct SpMeta {
    int64_t kept;                  // records before the cutoff
    int64_t bin_start1[257];
    int64_t tile_start2[257];
};
// Byte offsets of the partition buffers inside one workspace allocation.
struct SpLayout {
    size_t meta, comp1, val1, comp2, val2, cnt1, off1, cnt2, off2, leafflag, bounds, scan_tmp, scan_tmp_bytes,
        cur1, cur2, stat, big, curS, total;
};
SpPlan sparse_plan(const Batch& bt, int nb, int64_t rows);
// The one-level partition where it applies (compact fp32 plan, >= 8 pushes balanced
// over the slices, big leaves of 2 K - 8.7 K records on average): sets pl.big.
void sparse_plan_big(SpPlan& pl, const Batch& bt, int64_t rows);
// One 8-B word per fp32 record through the partition (SpPlan::compact): the row within
// its level-1 bin fits the word, and no ragged tail (compact words carry no sequence to
// cut at). Decided between sparse_plan and sparse_plan_big.
bool sparse_compact_ok(int vtype, const SpPlan& pl, bool has_tail_cut);
// Line buckets of the leaf kernels, bucket = (row - leaf's first row) >> bshift: the
// smallest shift that fits a leaf of 2^SL rows into k_sp_leaf's buckets, a big leaf of
// 2^BL rows into k_sp_leaf_big's.
int sparse_leaf_bshift(int SL);
int sparse_big_bshift(int BL);
hipError_t launch_sparse_partition_big(const Batch& bt, const SpPlan& pl, const SpLayout& l, uint8_t* ws,
                                       int64_t stride, int K, int64_t first, int64_t rows, Ctrl* ctrl,
                                       uint64_t tail_cut, SpStat* hstat, hipStream_t st);
SpLayout sparse_layout(const SpPlan& pl, int vbytes);
hipError_t launch_sparse_partition(int vtype, const Batch& bt, const SpPlan& pl, const SpLayout& l, uint8_t* ws,
                                   int64_t stride, int K, int64_t first, int64_t rows, Ctrl* ctrl,
                                   uint64_t tail_cut, hipStream_t st);
// Single-pass partition into the fixed-capacity layout; copies its SpStat to `hstat` (pinned).
hipError_t launch_sparse_partition_fast(int vtype, const Batch& bt, const SpPlan& pl, const SpLayout& l, uint8_t* ws,
                                        int64_t stride, int K, int64_t first, int64_t rows, Ctrl* ctrl,
                                        uint64_t tail_cut, SpStat* hstat, hipStream_t st);
// Sequence number of the first record at / past `cut` (a record-start position, or kNoPos).
uint32_t sparse_seq_cut(const SpPlan& pl, const Batch& bt, uint64_t cut, int64_t stride);
hipError_t launch_sparse_leaf(int vtype, void* shard, const SpPlan& pl, const SpLayout& l, uint8_t* ws, Ctrl* ctrl,
                              const Ctrl* prev, hipStream_t st, LaunchEv ev);
// Exact replay of the leaves the leaf kernel flagged. A compact chunk is first
// re-partitioned (counted, full sequence numbers) from its pushes.
hipError_t sparse_replay(int vtype, void* shard, const SpPlan& pl, const SpLayout& l, uint8_t* ws, const Batch& bt,
                         int64_t stride, int K, int64_t first, int64_t rows, Ctrl* ctrl, uint64_t tail_cut,
                         hipStream_t st);

// ---- launch shape of a dense reduce (dml_kernels.hip) ----
// Vector geometry of a value type: elements per 16-B vector, bytes per element.
struct VecGeom {
    int vec, elem;
    constexpr int chunk() const { return 64 * vec; }  // elements of one wave-wide 1-KiB chunk
    // the flat kernels' rows: whole vectors, under 4 KiB
    constexpr bool flat_row(int32_t cols) const { return cols % vec == 0 && (int64_t)cols * elem < 4096; }
};
constexpr VecGeom vec_geom(int vtype) { return vtype == kF64 ? VecGeom{2, 8} : VecGeom{4, 4}; }
// Rows a wave of the flat kernels owns: J 16-B vectors per lane over rows of nv vectors.
constexpr int rows_per_wave(int J, int nv) {
    const int r = J * 64 / (nv > 0 ? nv : 1);
    return r < 1 ? 1 : r > 16 ? 16 : r;
}
enum ReduceFamily : int { kFamReduce = 0, kFamRows = 1 };             // k_reduce, k_reduce_rows
enum StorePolicy : int { kStCached = 0, kStNt = 1, kStThrough = 2 };  // shard stores (k_reduce_rows' SNT)
// Everything launch_reduce decides from (value type, mode, width) for the kernels it
// picks by shape: one row of kReduceShapes (dml_kernels.hip) plus the facts derived from
// the width. The flat family is chosen per chunk (use_flat) and is not described here.
struct ReduceShape {
    ReduceFamily family;
    int group;      // k_reduce: pushes in flight per wave (G)
    int depth;      // k_reduce_rows: 1 = one push at a time, 3 = pair-packed load groups
    int cpw;        // consecutive 1-KiB chunks of a row per wave
    int rpw;        // neighbouring rows per wave
    int wpb;        // waves per block
    bool nt_loads;  // non-temporal record loads
    StorePolicy store;
    bool full;      // every chunk whole: no column masks
    int bpc;        // blocks-per-CU cap (unused dynamic LDS), 0 = none
    // derived by reduce_shape()
    int row;        // index in kReduceShapes
    int vec;        // elements per 16-B vector
    int32_t nchunks;  // 1-KiB chunks per row
    int32_t ngroups;  // waves per row (or per rpw rows)
    bool one_wave;  // one wave owns all of a row's chunks
};
ReduceShape reduce_shape(int vtype, int mode, int32_t cols);

// The most maxDelta candidates one AdaGrad apply writes (the candidate buffer's size).
int64_t reduce_blocks(int vtype, int64_t rows, int32_t cols);
// True when launch_reduce(vtype, mode, cols) runs k_reduce_rows in a plain-sum mode,
// which rewrites every slot it reads to -1 (the next batch's index then needs no memset).
bool reduce_clears_slots(int vtype, int mode, int32_t cols);
// The chunk's plain-sum reduce is k_reduce_flat (narrow dense rows), not k_reduce_rows.
bool use_flat(int vtype, int mode, int32_t cols, const Batch& bt, int nb, int64_t rows);
// k_flat_ident (dml_kernels.hip): a flat-shape chunk (use_flat, kAdd / kPreReduce)
// the host has seen, after its index, to be all identity — every push lists every
// row as record r = row r (flat_ident_ok), no cutoff, no repeated row. Its waves
// verify every key; a mismatch clears ctrl->spec_ok as k_reduce_flat does.
constexpr int kFlatIdentWaves = 8;  // waves per block (their rows written after one block barrier)
hipError_t launch_ada_ident(void* shard, int64_t rows, int32_t cols, const Batch& bt, int nb, int64_t stride, int K,
                            const AdaArgs& ada, hipStream_t st, int64_t* ncand_out, LaunchEv ev = {});
hipError_t launch_flat_ident(int vtype, int mode, void* shard, int64_t rows, int32_t cols, const Batch& bt, int nb,
                             int64_t stride, int K, Ctrl* ctrl, hipStream_t st, int64_t* nblocks_out,
                             LaunchEv ev = {}, RowMap rm = {});
// Whether a chunk of nb pushes may run k_flat_ident, from the host's copy of its
// Ctrl after the index (hctrl) and the pushes' record counts (`need` per push: the
// model rows).
bool flat_ident_ok(const Ctrl& hctrl, const Batch& bt, int nb, int64_t need, uint64_t tail_cut);
// Task rows per wave of k_flat_ident at this width (a row map's blocks must hold whole waves).
int flat_ident_rows_per_wave(int vtype, int32_t cols);
// row shapes whose reduce runs identity-speculative chunks (k_reduce_rows FULL, k_reduce_flat)
bool spec_shape(int vtype, int32_t cols);

uint64_t splitmix64(uint64_t x);

// Name of the dominant kernel (reduce / flat / AdaGrad / sparse leaf) the calling
// thread launched last, in rocprof's form, e.g.
// "dml::k_reduce_rows<float, 0, 4, 4, true, true, 1, 4, 2>": bench.py ties a profile's
// counted HBM bytes to the instantiation that ran (dml_store_kernel_name).
extern thread_local const char* g_kernel_name;
inline std::string kname_arg(bool v) { return v ? "true" : "false"; }
inline std::string kname_arg(int v) { return std::to_string(v); }
inline std::string kname_arg(const char* v) { return v; }
template <typename... A>
std::string kname(const char* base, A... a) {
    std::string s = std::string("dml::") + base + "<";
    bool first = true;
    ((s += (first ? "" : ", ") + kname_arg(a), first = false), ...);
    return s + ">";
}
template <typename T>
inline const char* type_name() {
    if constexpr (sizeof(T) == 8) return "double";
    else if constexpr (T(0.5) == T(0)) return "int";
    else return "float";
}

// Records `msg` as the calling thread's dml_last_error() and returns `code`
// (dml_store.hip; shared by the C-ABI translation units).
int set_error(int code, const std::string& msg);
// The store's side of a chained AdaGrad call, for the group (dml_store.hip): the commit
// of rows [row0, row0 + nrows) of the slice that came home (rec == null: the running
// maxDelta stays), and the device addresses of the delta plane and the running MaxDelta.
int store_assign_adagrad(dml_store* s, int64_t row0, int64_t nrows, const void* data, const void* delta,
                         const void* marks, const void* rec);
int store_adagrad_ptrs(dml_store* s, float** delta, void** maxdelta);
// The int32 store's side of a chained call, for the group: the device address of its
// sticky closed record (allocated open on first use), and the verdict of the commits
// enqueued so far (`block`: wait for the last one) — a closed record puts the store into
// its error state, DML_E_NEGATIVE_COUNTER with the record's key and col.
int store_chain_i32_record(dml_store* s, void** dev_rec);
int store_chain_i32_collect(dml_store* s, bool block);
// The store's side of a group pull (dml_store.hip): the handleFetch record's bytes, and the
// encode of keys that all lie inside the shard, enqueued on the apply stream whatever the
// entry's deferred error is (it is returned behind the launch).
int store_fetch_record_bytes(dml_store* s, int64_t* rec);
int store_pull_encode(dml_store* s, const int64_t* dev_keys, int64_t nkeys, void* dev_out);
// dml_pull.hip: the key partition and the record permutation of dml_group_pull.
size_t pull_partition_ws_bytes(int64_t n, int world);
hipError_t launch_pull_partition(const int64_t* keys, int64_t n, int64_t total_rows, int64_t step, int world,
                                 uint8_t* ws, int64_t* out_keys, int64_t* slot, int64_t* kept, int64_t* perm,
                                 int64_t* tot, hipStream_t st);
hipError_t launch_pull_unsplit(const void* src, const int64_t* perm, int64_t nrec, int64_t rec_bytes, void* dst,
                               int variant, hipStream_t st);

}  // namespace dml

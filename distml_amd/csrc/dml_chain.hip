// dml_chain.hip — the kernels of the chained reduce-scatter that are not a dense reduce
// (DESIGN.md §6). A chained step sums a travelling slice with this rank's pushes in push
// order; the plain-sum steps are launch_reduce's kChain / kChainCheckI32 modes
// (dml_kernels.hip), and this file holds what runs beside and after them.
//
//   k_chain_i32_verdict, k_chain_i32_merge  int32 matrices: kChainCheckI32 (k_reduce_rows /
//                   k_reduce) sums a step with the check after every add,
//                   k_reduce<kRollbackI32> undoes the adds past the first negative, the
//                   verdict closes the slice's record (IllegalStateException(key, col),
//                   IntMatrixStore.java:164-178), the merge closes the owner's
//   k_chain_ada_ident, k_chain_ada_rows, k_chain_ada_commit  AdaGrad matrices
//                   (FloatMatrixStoreAdaGrad.java:249-284): the step over the data and
//                   delta planes, touched marks and maxDelta candidates, and the owner's
//                   commit (one documented divergence, the alpha of an element whose delta
//                   comes home NaN — dml_group_push_exchange is the path without it)
//
// Compiled like every kernel file with -ffp-contract=off and IEEE denormals. The steps are
// driven by dml_prereduce.hip (dml_prereduce_chain_piece_ada, dml_prereduce_chain_close_i32),
// the commits by dml_store_owner.hip.
#include "dml_device.h"
#include "dml_launch.h"

#include <algorithm>
#include <climits>

namespace dml {

// ---------------------------------------------------------------------------
// Chained int32 step, after the slice's rollback: one wave, lane 0. Ctrl::neg_pos holds
// the earliest position at which one of this rank's adds left a counter of the slice
// negative (kChainCheckI32's atomicMin over every piece of the step), or kNoPos. A set
// word closes an open record: the position, the key of the record of the push that
// holds it, the column, the ring step (IllegalStateException(key, col),
// IntMatrixStore.java:174-176). The word is handed back as kNoPos for the next step.
__global__ __launch_bounds__(64) void k_chain_i32_verdict(const Batch bt, int nb, int64_t stride, int K,
                                                          Ctrl* __restrict__ ctrl, ChainI32Rec* __restrict__ rec,
                                                          int32_t step) {
    if (threadIdx.x != 0) return;
    const unsigned long long pos = ctrl->neg_pos;
    if (pos == kNoPos) return;
    ctrl->neg_pos = kNoPos;
    if (rec->pos != kNoPos) return;
    const int gb = (int)(pos >> 40);
    const uint64_t off = pos & kOffMask;
    int b = 0;
    for (int j = 0; j < nb; ++j) b = bt.bidx[j] == gb ? j : b;
    const int64_t r = (int64_t)(off / (uint64_t)stride);
    rec->key = ld_key(bt.base[b] + r * stride, K);
    rec->col = (int32_t)(((int64_t)off - r * stride - (int64_t)K) / 4);
    rec->step = step;
    rec->pad = 0ull;
    rec->pos = pos;
}

hipError_t launch_chain_i32_verdict(const Batch& bt, int nb, int64_t stride, int K, Ctrl* ctrl, ChainI32Rec* rec,
                                    int32_t step, hipStream_t st, LaunchEv ev) {
    return launch_k(k_chain_i32_verdict, dim3(1), dim3(64), 0, st, ev, bt, nb, stride, K, ctrl, rec, step);
}

// The owner's commit of a chained int32 slice: a closed home record closes the store's
// record, once (the first verdict stays: the store is in its error state from then on).
__global__ __launch_bounds__(64) void k_chain_i32_merge(ChainI32Rec* __restrict__ store_rec,
                                                        const ChainI32Rec* __restrict__ home) {
    if (threadIdx.x != 0) return;
    if (store_rec->pos == kNoPos && home->pos != kNoPos) *store_rec = *home;
}

hipError_t launch_chain_i32_merge(ChainI32Rec* store_rec, const ChainI32Rec* home, hipStream_t st) {
    hipLaunchKernelGGL(k_chain_i32_merge, dim3(1), dim3(64), 0, st, store_rec, home);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Chained reduce-scatter step of an AdaGrad matrix (dml_prereduce_chain_piece_ada,
// DESIGN.md §6): the slice travels as two planes, data and delta, plus one 4-byte
// touched mark per row. Task row t starts from base + t*cols in both planes; the
// handle's pushes' records of its model row are added in push order with the
// arithmetic of k_ada_ident / k_ada_flat (acc = acc + g, nd = dl + g*g, one IEEE
// rounding each), and both planes are written to the outputs (out == base works:
// every element and every mark is read and written by one lane). All pushes of the
// handle (up to 64) go through one pass: the planes are read once and written once
// whatever the push count, D push loads in flight per lane. No alpha is read or
// written: the owner computes it once from the delta that comes home
// (k_chain_ada_commit). An element's last strict rise of delta is its maxDelta
// candidate, reduced per block (max value, then lowest position) into ca.cand; a
// handle's pushes are numbered by column (dml_prereduce_begin: bidx[j] = j), so a
// candidate's position is formed from its push column. A row no push lists, a
// padding row, and every row of a handle whose index failed (ctrl_index_failed,
// read by every wave) are copied bit for bit, marks included; a listed row of a
// good handle sets its mark.
//
// k_chain_ada_ident: the vector stream for calls the host has seen to be all
// identity (ascending full-range pushes of a flat width, every key checked by
// k_ident_full before the first piece: config 4's shape). A thread owns one 16-B
// vector of the task planes; its model row goes through the row map per vector, so
// row blocks of any size work.
template <int D>
__global__ __launch_bounds__(256) void k_chain_ada_ident(int64_t nvec, int32_t cols, const Batch bt, int nb,
                                                         int64_t stride, int K, const Ctrl* __restrict__ ctrl,
                                                         RowMap rm, ChainAda ca) {
    constexpr int VEC = 4;
    const int64_t v = xcd_block() * 256 + threadIdx.x;
    const bool on = v < nvec;
    const int64_t e0 = on ? v * VEC : 0;
    const int64_t t = e0 / cols;
    const int c = (int)(e0 - t * cols);
    const int64_t mr = rm.row(t);
    const bool live = on && mr < rm.rows_total && !ctrl_index_failed(ctrl);
    const int64_t roff = mr * stride + K + (int64_t)c * 4;
    const u32x4 z{0u, 0u, 0u, 0u};
    float acc[VEC], dl[VEC], rv[VEC];
    int rb[VEC];  // push of the element's last strict rise (-1: none)
    unpack<float>(on ? ldg16_nt((const uint8_t*)rm.base + e0 * 4) : z, acc);
    unpack<float>(on ? ldg16_nt((const uint8_t*)ca.base_delta + e0 * 4) : z, dl);
    uint32_t mark = 0u;
    if (on && c == 0 && ca.base_marks) mark = ca.base_marks[t];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        rv[e] = 0.f;
        rb[e] = -1;
    }
#pragma unroll 1
    for (int b0 = 0; b0 < nb; b0 += D) {
        u32x4 raw[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int b = b0 + d < nb ? b0 + d : b0;
            raw[d] = live && b0 + d < nb ? ldg16_nt(bt.base[b] + roff) : z;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (b0 + d >= nb || !live) continue;
            float g[VEC];
            unpack<float>(raw[d], g);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                acc[e] = __fadd_rn(acc[e], g[e]);
                const float nd = __fadd_rn(dl[e], __fmul_rn(g[e], g[e]));
                if (nd > dl[e]) { rv[e] = nd; rb[e] = b0 + d; }
                dl[e] = nd;
            }
        }
    }
    float cand_v = 0.f;
    uint64_t cand_p = kNoPos;
    bool cand_ok = false;
    if (on) {
        stg16_nt((uint8_t*)rm.out + e0 * 4, pack<float>(acc));
        stg16_nt((uint8_t*)ca.out_delta + e0 * 4, pack<float>(dl));
        if (c == 0) ca.out_marks[t] = live ? 1u : mark;
        // (push, element) order is position order inside the thread's vector
        int key = 0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (rb[e] < 0) continue;
            const int k = (rb[e] << 2) | e;
            if (!cand_ok || rv[e] > cand_v || (rv[e] == cand_v && k < key)) {
                cand_ok = true;
                cand_v = rv[e];
                key = k;
            }
        }
        if (cand_ok) cand_p = pos_of((uint64_t)(key >> 2), (uint64_t)(roff + (key & 3) * 4));
    }
    cand_block_best<4>(cand_ok, cand_v, cand_p);
    if (threadIdx.x == 0) ca.cand[blockIdx.x] = cand_of(cand_ok, cand_v, cand_p);
}

// k_chain_ada_rows: the slot-table shape for everything else (permuted pushes, ragged
// or narrow rows, rows no push lists): one wave per task row, its lanes over the
// row's columns 64 at a time, element by element (any width, 4-byte aligned records).
// The row's slots (one per push; slot = row for a push k_ident_full confirmed) are
// read once into LDS and handed back clean (-1), as the pre-reduce kernels do.
template <int D>
__global__ __launch_bounds__(256) void k_chain_ada_rows(int64_t ntask, int32_t cols, const Batch bt, int nb,
                                                        int64_t stride, int K, int32_t* __restrict__ slot,
                                                        const Ctrl* __restrict__ ctrl, RowMap rm, ChainAda ca) {
    __shared__ int32_t s_slot[4][kMaxW];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t t = (int64_t)blockIdx.x * 4 + wid;
    const bool on = t < ntask;
    const int64_t mr = on ? rm.row(t) : 0;
    const bool good = on && mr < rm.rows_total && !ctrl_index_failed(ctrl);
    const uint64_t ident = bt.ident_ok ? ctrl->ident : 0ull;
    const int ss = slot_stride(nb);
    int32_t* const ls = s_slot[wid];
    int32_t sl = -1;
    if (good && lane < nb) {
        if ((ident >> lane) & 1ull) {
            sl = (int32_t)mr;  // a confirmed push is full-range: record r is row r
        } else {
            sl = slot[mr * ss + lane];
            if (sl >= 0) slot[mr * ss + lane] = -1;
        }
    }
    ls[lane] = sl;
    wave_lds_handover();
    const bool live = __ballot(sl >= 0) != 0ull;  // some push lists the row
    float cand_v = 0.f;
    uint64_t cand_p = kNoPos;
    bool cand_ok = false;
    const float* const bd = (const float*)rm.base;
    float* const od = (float*)rm.out;
    for (int c0 = 0; c0 < cols; c0 += 64) {
        const int c = c0 + lane;
        const bool act = on && c < cols;
        const int64_t i = act ? t * (int64_t)cols + c : 0;
        float acc = 0.f, dl = 0.f, rv = 0.f;
        int rb = -1;
        if (act) {
            acc = bd[i];
            dl = ca.base_delta[i];
        }
        if (live) {
#pragma unroll 1
            for (int b0 = 0; b0 < nb; b0 += D) {
                int32_t s[D];
                float g[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int b = b0 + d < nb ? b0 + d : b0;
                    s[d] = b0 + d < nb ? __builtin_amdgcn_readfirstlane(ls[b]) : -1;
                    g[d] = act && s[d] >= 0
                               ? Elem<float>::load(bt.base[b] + (int64_t)s[d] * stride + K + (int64_t)c * 4)
                               : 0.f;
                }
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    if (s[d] < 0 || !act) continue;
                    acc = __fadd_rn(acc, g[d]);
                    const float nd = __fadd_rn(dl, __fmul_rn(g[d], g[d]));
                    if (nd > dl) { rv = nd; rb = b0 + d; }
                    dl = nd;
                }
            }
        }
        if (act) {
            od[i] = acc;
            ca.out_delta[i] = dl;
            if (rb >= 0) {
                const uint64_t p = pos_of((uint64_t)rb, (uint64_t)((int64_t)ls[rb] * stride + K + (int64_t)c * 4));
                if (cand_better(true, rv, p, cand_ok, cand_v, cand_p)) {
                    cand_ok = true;
                    cand_v = rv;
                    cand_p = p;
                }
            }
        }
    }
    if (on && lane == 0) ca.out_marks[t] = live ? 1u : (ca.base_marks ? ca.base_marks[t] : 0u);
    cand_block_best<4>(cand_ok, cand_v, cand_p);
    if (threadIdx.x == 0) ca.cand[blockIdx.x] = cand_of(cand_ok, cand_v, cand_p);
}

constexpr int kChainAdaD = 8;  // push loads in flight per lane

int64_t chain_ada_blocks(bool ident, int64_t ntask, int32_t cols) {
    return ident ? (ntask * (cols / 4) + 255) / 256 : (ntask + 3) / 4;
}

hipError_t launch_chain_ada(bool ident, int64_t ntask, int32_t cols, const Batch& bt, int nb, int64_t stride, int K,
                            int32_t* slot, const Ctrl* ctrl, RowMap rm, const ChainAda& ca, hipStream_t st,
                            int64_t* ncand_out, LaunchEv ev) {
    if (!rm.base || !rm.out || !ca.base_delta || !ca.out_delta || !ca.out_marks || !ca.cand)
        return hipErrorInvalidValue;
    if (ident && (cols % 4 || nb <= 0)) return hipErrorInvalidValue;
    const int64_t nblocks = chain_ada_blocks(ident, ntask, cols);
    if (nblocks > INT32_MAX) {
        if (ncand_out) *ncand_out = nblocks;
        return hipErrorInvalidValue;
    }
    constexpr int D = kChainAdaD;
    if (ident)
        return launch_named<k_chain_ada_ident<D>>(std::make_tuple("k_chain_ada_ident", D), nblocks, ncand_out, 256, 0, st,
                                                  ev, ntask * (cols / 4), cols, bt, nb, stride, K, ctrl, rm, ca);
    return launch_named<k_chain_ada_rows<D>>(std::make_tuple("k_chain_ada_rows", D), nblocks, ncand_out, 256, 0, st, ev,
                                             ntask, cols, bt, nb, stride, K, slot, ctrl, rm, ca);
}

// The owner's commit of its AdaGrad slice when the chain brings it home: shard data
// and delta = the slice's; alpha = initialAlpha / (factor * sqrt(delta)), clamped to
// minAlpha (k_ada_ident's expression, the owner's parameters), where the row's mark is
// set and delta > 1 — inside one call delta never falls, so this is the alpha the
// reference's last update of the element left (FloatMatrixStoreAdaGrad.java:268-272).
// A NaN delta fails the comparison: such an element keeps the alpha the owner held
// (the one documented divergence). The store's running maxDelta
// becomes the travelling record.
__global__ __launch_bounds__(256) void k_chain_ada_commit(float* __restrict__ data, float* __restrict__ delta,
                                                          float* __restrict__ alpha, MaxDelta* __restrict__ md,
                                                          const float* __restrict__ sdata,
                                                          const float* __restrict__ sdelta,
                                                          const uint32_t* __restrict__ marks,
                                                          const MaxDelta* __restrict__ rec, int64_t n, int32_t cols,
                                                          float initial_alpha, float min_alpha, float factor) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = sdelta[i];
        data[i] = sdata[i];
        delta[i] = d;
        if (d > 1.0f && marks[i / cols] != 0u) alpha[i] = ada_alpha(d, initial_alpha, factor, min_alpha);
    }
    if (md && blockIdx.x == 0 && threadIdx.x == 0) {
        md->value = rec->value;
        md->row = rec->row;
        md->col = rec->col;
    }
}

hipError_t launch_chain_ada_commit(float* data, float* delta, float* alpha, MaxDelta* md, const float* sdata,
                                   const float* sdelta, const uint32_t* marks, const MaxDelta* rec, int64_t rows,
                                   int32_t cols, const AdaArgs& ada, hipStream_t st) {
    const int64_t n = rows * cols;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 8192));
    hipLaunchKernelGGL(k_chain_ada_commit, dim3(grid), dim3(256), 0, st, data, delta, alpha, md, sdata, sdelta, marks,
                       rec, n, cols, ada.initial_alpha, ada.min_alpha, ada.factor);
    return hipGetLastError();
}

}  // namespace dml

// dml_moments.hip — the two-moment AdaGrad path of a sharded matrix.
//
//   k_moments_flat    a rank's pre-reduce piece: Σu and Σu·u per element of its pushes
//   k_ada_moments     the owner's apply of the reduce-scattered moments: data, delta,
//                     alpha, one maxDelta candidate per block
//   k_maxdelta_elems  the finalize of those element-index candidates
//
// The update they reproduce is FloatMatrixStoreAdaGrad.java:262-277, in another summation
// order (within 1e-6 of it, not bit-exact; tests pin the kernels bit for bit to a
// push-order model instead). The pieces are driven by dml_prereduce.hip
// (dml_prereduce_moments_piece), the apply by dml_store_owner.hip.
#include "dml_device.h"
#include "dml_launch.h"

namespace dml {

// ---------------------------------------------------------------------------
// Two-moment AdaGrad reduce-scatter: the sharded
// AdaGrad path whose xGMI bytes do not grow with the pushes per rank. Each rank
// pre-reduces its full-range pushes into Σu and Σu·u per element (fp32, push
// order; u·u rounded, then added, like the reference's delta update,
// FloatMatrixStoreAdaGrad.java:265-267), written as one [row][2 x cols] run so a
// rank's share of both is one contiguous reduce-scatter chunk; the owner applies
// row += Σu, delta += Σu², and alpha = f(final delta) where it ends above 1
// (:268-272: delta never falls, so the last push that sets alpha sees the final
// delta). The summation order is not the reference's: within 1e-6, not bit-exact.
//
// k_moments_flat: k_reduce_flat's layout (R rows per wave as one flat run of
// 16-B vectors), slot rows in LDS unless every push is identity (Batch::ident_ok).
// A call whose index met a key outside the matrix or a repeated row writes zeros
// (dml_prereduce_end reports the error; nothing of it is applied).
template <int JMAX>
__global__ __launch_bounds__(256) void k_moments_flat(int64_t ntask, int32_t cols, int32_t R, const Batch bt, int nb,
                                                      int64_t stride, int K, int32_t* __restrict__ slot,
                                                      const Ctrl* __restrict__ ctrl, RowMap rm) {
    constexpr int VEC = 4;
    constexpr int RMAX = 16;
    __shared__ int32_t s_slot[4][RMAX * kMaxW];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t t0 = (xcd_block() * 4 + wid) * R;  // first task row of the wave (XCD-contiguous, as k_reduce_flat)
    if (t0 >= ntask) return;
    const int NV = cols / VEC;
    const int nrow = (int)(ntask - t0 < (int64_t)R ? ntask - t0 : (int64_t)R);
    const int ss = slot_stride(nb);
    int32_t* const ls = s_slot[wid];
    const uint64_t ident = bt.ident_ok ? ctrl->ident : 0ull;
    const uint64_t nbm = nb >= 64 ? ~0ull : (1ull << nb) - 1ull;
    const bool all_id = (ident & nbm) == nbm;
    const bool err = ctrl->cutoff != kNoPos || ctrl->no_dup == 0u;
    const int64_t lrow = rm.row(t0 + lane);
    const uint32_t padm = (uint32_t)__ballot(lane < nrow && lrow >= rm.rows_total);
    if (!all_id) {
        // slot rows into LDS, handed back clean (-1) like k_reduce_flat's
        for (int e = lane; e < nrow * nb; e += 64) {
            const int rl = e / nb, b = e - rl * nb;
            const int64_t mr = rm.row(t0 + rl);
            int32_t v = -1;
            if (!((padm >> rl) & 1u)) {
                if ((ident >> b) & 1ull) {
                    v = mr < bt.nrec[b] ? (int32_t)mr : -1;
                } else {
                    v = slot[mr * ss + b];
                    if (v >= 0) slot[mr * ss + b] = -1;
                }
            }
            ls[rl * kMaxW + b] = v;
        }
        wave_lds_handover();
    }
    int rc[JMAX];
    uint32_t on = 0;
    float acc[JMAX][VEC], sq[JMAX][VEC];
    const int nvec = nrow * NV;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        const int v = j * 64 + lane;
        const int rlj = v < nvec ? v / NV : 0;
        const int cvj = v < nvec ? v - rlj * NV : 0;
        rc[j] = (rlj << 16) | cvj;
        on |= ((v < nvec && !((padm >> rlj) & 1u) && !err) ? 1u : 0u) << j;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[j][e] = sq[j][e] = 0.f;
    }
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const uint8_t* const bp = bt.base[b];
        int32_t rr[JMAX];
        u32x4 raw[JMAX];
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            const int rl = rc[j] >> 16;
            rr[j] = (on >> j & 1u) ? (all_id ? (int32_t)rm.row(t0 + rl) : ls[rl * kMaxW + b]) : -1;
            raw[j] = rr[j] >= 0 ? ldg16_nt(bp + (int64_t)rr[j] * stride + K + (int64_t)(rc[j] & 0xFFFF) * 16)
                                : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (rr[j] < 0) continue;
            float u[VEC];
            unpack<float>(raw[j], u);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                acc[j][e] = __fadd_rn(acc[j][e], u[e]);
                sq[j][e] = __fadd_rn(sq[j][e], __fmul_rn(u[e], u[e]));
            }
        }
    }
    float* const out = (float*)rm.out;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        if (j * 64 + lane >= nvec) continue;
        float* const op = out + (t0 + (rc[j] >> 16)) * (int64_t)(2 * cols) + (rc[j] & 0xFFFF) * VEC;
        stg16(op, pack<float>(acc[j]));
        stg16(op + cols, pack<float>(sq[j]));
    }
}

hipError_t launch_moments(int64_t ntask, int32_t cols, const Batch& bt, int nb, int64_t stride, int K, int32_t* slot,
                          const Ctrl* ctrl, RowMap rm, hipStream_t st, LaunchEv ev) {
    constexpr int JMAX = 8;
    if (!vec_geom(kF32).flat_row(cols) || !rm.out) return hipErrorInvalidValue;  // the flat shapes
    const int R = rows_per_wave(JMAX, cols / 4);
    return launch_named<k_moments_flat<JMAX>>(std::make_tuple("k_moments_flat", JMAX), flat_blocks(ntask, R, 4), nullptr,
                                              256, 0, st, ev, ntask, cols, R, bt, nb, stride, K, slot, ctrl, rm);
}

// Owner apply of the reduce-scattered moments ([row][Σu | Σu²], rows x 2 cols):
// data += Σu, delta += Σu², alpha = f(delta) where delta ends above 1, each
// element's strict rise of delta its maxDelta candidate (ties: first in row-major
// order). One candidate per block into ada.cand.
__global__ __launch_bounds__(256) void k_ada_moments(float* __restrict__ shard, const float* __restrict__ src,
                                                     int64_t rows, int32_t cols, AdaArgs ada) {
    const int NV = cols / 4;
    const int64_t nvec = rows * NV;
    float cand_v = 0.f;
    uint64_t cand_p = kNoPos;
    bool cand_ok = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / NV;
        const int cv = (int)(i - r * NV);
        const int64_t ei = r * cols + cv * 4;
        const float* sp = src + r * (int64_t)(2 * cols) + cv * 4;
        float a[4], d[4], su[4], s2[4];
        unpack<float>(ldg16_nt((const uint8_t*)(shard + ei)), a);
        unpack<float>(ldg16_nt((const uint8_t*)(ada.delta + ei)), d);
        unpack<float>(ldg16((const uint8_t*)sp), su);
        unpack<float>(ldg16((const uint8_t*)(sp + cols)), s2);
        float na[4];
        bool all_a = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = __fadd_rn(a[e], su[e]);
            const float nd = __fadd_rn(d[e], s2[e]);
            if (nd > d[e] && (!cand_ok || nd > cand_v)) {  // elements visited in row-major order per thread
                cand_ok = true;
                cand_v = nd;
                cand_p = (uint64_t)(ei + e);
            }
            d[e] = nd;
            na[e] = 0.f;
            if (nd > 1.0f) {
                // ada_alpha(), restated: the call changes this kernel's code
                na[e] = (float)((double)ada.initial_alpha / ((double)ada.factor * sqrt((double)nd)));
                if (na[e] < ada.min_alpha) na[e] = ada.min_alpha;
            } else {
                all_a = false;
            }
        }
        stg16_nt(shard + ei, pack<float>(a));
        stg16_nt(ada.delta + ei, pack<float>(d));
        if (all_a) {
            stg16_nt(ada.alpha + ei, pack<float>(na));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (d[e] > 1.0f) ada.alpha[ei + e] = na[e];
        }
    }
    cand_block_best<4>(cand_ok, cand_v, cand_p);
    if (threadIdx.x == 0) ada.cand[blockIdx.x] = cand_of(cand_ok, cand_v, cand_p);
}

// maxDelta finalize for element-index candidates (k_ada_moments): the reference's
// strict `>` against the running maximum; row = the element's key (first + row).
__global__ __launch_bounds__(256) void k_maxdelta_elems(const DeltaCand* __restrict__ cand, int64_t n,
                                                        MaxDelta* __restrict__ md, int64_t first, int32_t cols) {
    bool ok = false;
    float v = 0.f;
    uint64_t p = kNoPos;
    cand_scan(cand, threadIdx.x, n, 256, ok, v, p);
    cand_block_best<4>(ok, v, p);
    if (threadIdx.x != 0) return;
    if (ok && v > md->value) {
        md->value = v;
        md->row = (int32_t)(first + (int64_t)(p / (uint64_t)cols));
        md->col = (int32_t)(p % (uint64_t)cols);
    }
}

hipError_t launch_ada_moments(float* shard, const float* src, int64_t rows, int32_t cols, const AdaArgs& ada,
                              MaxDelta* md, int64_t first, hipStream_t st, LaunchEv ev) {
    if (cols % 4 || rows <= 0) return hipErrorInvalidValue;
    g_kernel_name = "dml::k_ada_moments";
    const hipError_t e = launch_k(k_ada_moments, dim3(kMomentBlocks), dim3(256), 0, st, ev, shard, src, rows, cols, ada);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_maxdelta_elems, dim3(1), dim3(256), 0, st, ada.cand, (int64_t)kMomentBlocks, md, first, cols);
    return hipGetLastError();
}

}  // namespace dml

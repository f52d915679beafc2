// dml_launch.h — host-side launch helpers the kernel files share (dml_kernels.hip,
// dml_chain.hip, dml_moments.hip, dml_ops.hip, dml_diag.hip). Host only; what the kernels
// themselves share is dml_device.h. Not part of the public ABI.
#pragma once
#include "dml_internal.h"

#include <hip/hip_ext.h>

#include <string>
#include <tuple>

namespace dml {

// Occupancy cap: dynamic LDS (unused by the kernels) so that at most `bpc`
// 256-thread blocks fit on a CU (160 KiB of LDS per CU). 0 = no cap.
constexpr unsigned kLdsPerCU = 160 * 1024;
inline unsigned lds_for_blocks_per_cu(int bpc) { return bpc > 0 ? kLdsPerCU / (unsigned)(bpc + 1) + 256u : 0u; }

// One launch of `kernel`: its start / stop events ride in the dispatch packet when the
// caller carries any (hipExtLaunchKernel); a plain launch otherwise.
template <typename... KA, typename... A>
static inline hipError_t launch_k(void (*kernel)(KA...), dim3 grid, dim3 block, unsigned lds, hipStream_t st,
                                  LaunchEv ev, const A&... a) {
    if (ev.start || ev.stop)
        hipExtLaunchKernelGGL(kernel, grid, block, lds, st, ev.start, ev.stop, 0, static_cast<KA>(a)...);
    else
        hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<KA>(a)...);
    return hipGetLastError();
}

// One launch of KERNEL over `nblocks` blocks of `threads`, as the dominant kernel of the
// calling thread: reports the grid (`nblocks_out`, may be null), returns on an empty one,
// and otherwise records the instantiation's name, formed once from `name` (kname's
// arguments: base name, then the template arguments), as g_kernel_name.
template <auto KERNEL, typename... N, typename... A>
static inline hipError_t launch_named(const std::tuple<const char*, N...>& name, int64_t nblocks, int64_t* nblocks_out,
                                      unsigned threads, unsigned lds, hipStream_t st, LaunchEv ev, const A&... a) {
    if (nblocks_out) *nblocks_out = nblocks;
    if (nblocks <= 0) return hipSuccess;
    static const std::string kn = std::apply([](auto... n) { return kname(n...); }, name);
    g_kernel_name = kn.c_str();
    return launch_k(KERNEL, dim3((unsigned)nblocks), dim3(threads), lds, st, ev, a...);
}

// Grid of a grid-stride kernel over n items, 256 per block.
static inline unsigned grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    return (unsigned)(g < 1 ? 1 : g);
}

// Blocks of a flat launch: R rows per wave, nw waves per block.
static inline int64_t flat_blocks(int64_t rows, int R, int nw) { return ((rows + R - 1) / R + nw - 1) / nw; }

}  // namespace dml

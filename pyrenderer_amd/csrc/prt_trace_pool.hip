// prt_trace_pool.hip — the block-pooled shadow-query trace kernel (prt_pool.h trace_kernel_pool)
// in its own compilation unit: pyrenderer_amd/build.py compiles it with LLVM's AMDGPU
// register-pressure trackers (-mllvm --amdgpu-use-amdgpu-trackers), under which the kernel fits
// the 72 VGPRs of 7 waves per SIMD with 3 spilled registers instead of 39 (the other trace
// kernels keep the default scheduler: the global-scene kernel is slower with the trackers,
// DESIGN.md §2).  One schedule: extension traversals, then the pooled shadow rays in 64-ray
// chunks after the block barrier (round 5's fused, packed-leaf and split-arrival schedules were
// removed in round 6: none became the default).
// PRT_POOL_WIDTH (4 when not defined, or 8): the children per node of the LDS-resident tree the unit's
// kernels traverse; build.py compiles this file once per width.
#pragma clang fp contract(off)

#include "prt_device.h"

#ifndef PRT_POOL_WIDTH
#define PRT_POOL_WIDTH 4
#endif
#define PRT_CAT2(a, w) a##w
#define PRT_CAT(a, w) PRT_CAT2(a, w)

namespace prt {

namespace {
constexpr int kW = PRT_POOL_WIDTH;
template <bool STATS, int WPE>
hipError_t launch_pool(const TraceParams& P, int grid, size_t smem, hipStream_t stream) {
    if (P.plain) trace_kernel_pool<STATS, WPE, true, kW><<<grid, kBlock, smem, stream>>>(P);
    else trace_kernel_pool<STATS, WPE, false, kW><<<grid, kBlock, smem, stream>>>(P);
    return hipGetLastError();
}
}  // namespace

hipError_t PRT_CAT(launch_trace_pool, PRT_POOL_WIDTH)(const TraceParams& P, bool stats, int wpe, int grid, size_t smem,
                                                      hipStream_t stream) {
    if (wpe != 7 && wpe != 6) return hipErrorInvalidValue;
    if (stats)
        return wpe == 7 ? launch_pool<true, 7>(P, grid, smem, stream) : launch_pool<true, 6>(P, grid, smem, stream);
    return wpe == 7 ? launch_pool<false, 7>(P, grid, smem, stream) : launch_pool<false, 6>(P, grid, smem, stream);
}

// both builds of one (stats, waves per EU) fit the same blocks per CU (the waves-per-EU target and
// the LDS size set it)
int PRT_CAT(trace_occ_pool, PRT_POOL_WIDTH)(bool stats, int wpe, size_t smem) {
    int n = 0;
    if (stats && wpe == 7)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel_pool<true, 7, false, kW>, kBlock, smem);
    else if (stats && wpe == 6)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel_pool<true, 6, false, kW>, kBlock, smem);
    else if (wpe == 7)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel_pool<false, 7, false, kW>, kBlock, smem);
    else if (wpe == 6)
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel_pool<false, 6, false, kW>, kBlock, smem);
    return n;
}

}  // namespace prt

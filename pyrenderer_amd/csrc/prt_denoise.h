// prt_denoise.h — launch interface of the edge-avoiding a-trous filter (prt_denoise.hip), shared
// with its C-ABI unit (prt_denoise_capi.cpp).  Not part of the trace kernels' sources: nothing here
// is included by them (pyrenderer_amd/build.py AUX_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace prt_dn {

constexpr int kMaxIterations = 8;
constexpr int kMaxSide = 32768;   // W, H: the launch grids and the 5-tap reach at step 128 stay in int

struct Params {
    float sigma_c, sigma_z, eps_a, eps_z;
};

// scratch of one W x H frame: two (I.rgb, Z) ping-pong planes and the (N.xyz, class) plane as
// float4, the depth-gradient plane as float2 — 56 bytes per pixel, rounded up to 256
size_t work_bytes(int W, int H);

// Enqueue pre-pass, `iterations` a-trous passes and the post-pass on `stream` of the current
// device.  All pointers are device pointers; d_work holds work_bytes(W, H) bytes, 16-byte aligned.
// Returns the first launch error.
hipError_t enqueue(const float* d_color, const float* d_feat, int W, int H, int iterations, const Params& p,
                   float* d_out, void* d_work, hipStream_t stream);

}  // namespace prt_dn

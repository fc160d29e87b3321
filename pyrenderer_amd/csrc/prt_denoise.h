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

// ---- variance-guided mode: the colour edge-stopping width follows the image's own noise ----
struct VarParams {
    float sigma_l, sigma_z, eps_a, eps_z, eps_l;
};

// scratch of one W x H frame: two (I.rgb, var) ping-pong planes and the (N.xyz, class) plane as
// float4, the depth-gradient plane as float2, the depth plane as float — 60 bytes per pixel,
// rounded up to 256
size_t var_work_bytes(int W, int H);

// Enqueue pre-pass, variance estimate, `iterations` variance-guided passes and the post-pass on
// `stream` of the current device.  d_out_var (W x H floats, may be null) receives the variance
// estimate of the demodulated luminance, before any pass; d_work holds var_work_bytes(W, H) bytes,
// 16-byte aligned.  Returns the first launch error.
//
// Finiteness: the variance planes are always finite (a variance that is not becomes 0, which is
// what an overflow of l * l, |l| >= 2^64, ends in).  Every colour of a pixel that is not set aside
// is finite while the demodulated radiance |C_c / fmax(A_c, eps_a)| <= 2^126 and the albedo
// A_c <= 1: the luminance and the difference of two luminances then stay finite, so no weight is
// inf / inf, and a weighted mean of such values times the albedo stays in range.
hipError_t enqueue_var(const float* d_color, const float* d_feat, int W, int H, int iterations, const VarParams& p,
                       float* d_out, float* d_out_var, void* d_work, hipStream_t stream);

}  // namespace prt_dn

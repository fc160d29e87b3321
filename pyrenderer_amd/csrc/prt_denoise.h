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

// Where the colour edge-stopping width comes from.  kFixed: sigma_c, halved every pass.  The other three are
// the variance-guided mode, whose width follows the image's own noise: kEstimate takes the variance from
// the 7 x 7 window, kGiven from the caller's plane d_in_var, and kMixed from that plane where it is finite
// and >= 0 and from the window elsewhere (SVGF's spatial fallback where a temporal history is too short).
enum class Mode { kFixed, kEstimate, kGiven, kMixed };

// sigma is sigma_c (kFixed) or sigma_l (the variance-guided modes); eps_l is read by the latter only
struct FilterParams {
    float sigma, sigma_z, eps_a, eps_z, eps_l;
};

// Scratch of one W x H frame, rounded up to 256 bytes.  Fixed filter: two (I.rgb, Z) ping-pong planes and
// the (N.xyz, class) plane as float4, the depth-gradient plane as float2: 56 bytes per pixel.
// `variance`: the ping-pong planes hold (I.rgb, var) and a float plane holds the depth: 60 bytes per pixel.
size_t work_bytes(int W, int H, bool variance);

// Enqueue the pre-pass, the mode's variance step (none for kFixed), `iterations` a-trous passes and the
// post-pass on `stream` of the current device.  All pointers are device pointers; d_work holds
// work_bytes(W, H, mode != kFixed) bytes, 16-byte aligned.  Returns the first launch error.
//
// d_out_var (W x H floats, may be null; not read for kFixed) receives the variance of the demodulated
// luminance that the passes start from, the variance actually used.
//
// d_in_var (W x H floats; required for kGiven and kMixed, not read otherwise) is a variance from outside,
// e.g. from per-pixel sample moments or a temporal state.  At a usable pixel a value that is finite and
// >= 0 is taken as it is (a -0 too); anything else counts as 0 for kGiven and keeps the window's estimate
// for kMixed, which the estimate's kernel selects in the same launch.  d_in_var must not alias d_out or
// d_out_var.
//
// Finiteness: the variance planes are always finite (a variance that is not becomes 0, which is
// what an overflow of l * l, |l| >= 2^64, ends in).  Every colour of a pixel that is not set aside
// is finite while the demodulated radiance |C_c / fmax(A_c, eps_a)| <= 2^126 and the albedo
// A_c <= 1: the luminance and the difference of two luminances then stay finite, so no weight is
// inf / inf, and a weighted mean of such values times the albedo stays in range.
hipError_t enqueue_filter(Mode mode, const float* d_color, const float* d_feat, const float* d_in_var, int W, int H,
                          int iterations, const FilterParams& p, float* d_out, float* d_out_var, void* d_work,
                          hipStream_t stream);

// ---- temporal accumulation ----
constexpr int kTemporalChannels = 8;   // I.rgb, h, m1, m2, var, 0: two float4 per pixel
struct TemporalParams {
    float alpha, alpha_m, tau_n, tau_z, tau_a, eps_a, min_history, w_min;
};

// Per-object motion.  ids / prev_ids: W x H int32 [x][y], this frame's and the previous frame's object id per
// pixel (prev_ids null on the first frame, with the other prev pointers).  rows: n_objects x 12 floats, per
// object the row-major 3 x 4 matrix that takes a world position of this frame to the same material point's
// position in the previous frame; not read when n_objects is 0, where it may be null.
constexpr int kMaxObjects = 1 << 20;
struct Motion {
    const int32_t* ids;
    const int32_t* prev_ids;
    const float* rows;
    int n_objects;
};

// Enqueue temporal_kernel on `stream` of the current device: this frame's mean radiance d_color (W x H x 3)
// and features d_feat (W x H x 8) blended into the previous frame's state, reprojected from the previous
// camera (tests/temporal_ref.py restates it).  cam24 / prev_cam24 are HOST pointers to the 24-float records
// (read before the call returns); d_prev_feat, prev_cam24 and d_prev_state are all null on the first frame.
// cameras_equal: the two records are bytewise equal.  d_state and d_prev_state hold W x H x 8 floats,
// 16-byte aligned, and must not be the same plane (taps read neighbours); d_out_color (W x H x 3,
// re-modulated) and d_out_var (W x H, the state's variance plane) may be null.
//
// motion: null is the static world (temporal_kernel<false>): with equal cameras every pixel reads its own
// previous state.  Otherwise its device pointers go to temporal_kernel<true>, the table's only when n_objects
// > 0.  An id outside 0..n_objects-1 has no row: its pixel reprojects as the static world's does and no table
// entry is read for it.  A row with an entry that is not finite means "no previous pose": the pixel starts
// afresh.  A tap counts only if its previous id equals the pixel's id.  With equal cameras a pixel takes its
// own previous state alone if its id has no row or the row is bytewise the identity.
//
// Finiteness: a pixel that takes part has finite colour, demodulated colour and features.  Its state is
// finite while |I_c| <= 2^62: the luminance and its square, the blends between two such values and the
// variance then stay in range.  The variance plane holds a quiet NaN wherever the history is shorter
// than min_history: prt_denoise_var_mixed reads it as "estimate here".  A finite row times a finite position
// may overflow to inf or NaN, which fails the range test of the projection (a comparison with a NaN is false)
// before any index is formed, so the pixel starts afresh.
hipError_t enqueue_temporal(const float* d_color, const float* d_feat, const float* cam24, const float* d_prev_feat,
                            const float* prev_cam24, const float* d_prev_state, const Motion* motion, int W, int H,
                            bool cameras_equal, const TemporalParams& p, float* d_state, float* d_out_color,
                            float* d_out_var, hipStream_t stream);

// ---- variance from per-pixel sample moments ----

// Running Welford update of the demodulated luminance over n_frames frames of per-pixel radiance sums
// (frame f at d_sums + f * frame_pitch floats, W x H x 3, each the sum of n_samples samples).
// d_io_state: W x H x 4 floats (k, mean, M2, var_mean), 16-byte aligned; zeroes are the empty state.
//
// Finiteness: a frame whose luminance l is not finite is skipped.  With |l| <= B, |mean| <= B, so both
// factors of d * (l - mean') are at most 2B and the product at most 4B^2; M2, a sum of k such
// non-negative terms, is at most k * B^2 in exact arithmetic.  The whole state is finite while
// k * B^2 <= 2^127: |l| <= 2^62 for up to 8 batches, |l| <= 2^51 for the 2^24 that k counts exactly.
// Beyond it M2 becomes inf and stays inf; var_mean is then stored as 0.
hipError_t enqueue_moments(const float* d_sums, int n_frames, size_t frame_pitch, float n_samples, const float* d_feat,
                           float eps_a, int W, int H, float* d_io_state, hipStream_t stream);

// ---- adaptive sampling ----
constexpr int kMinTilePixels = 64, kMaxTilePixels = 1 << 20;   // tw * th, the render calls' rule

struct AdaptiveParams {
    float n_samples, eps_a, eps_r, target;
};

// Enqueue adaptive_kernel on `stream` of the current device: one batch of the tiles `tile_ids` (d_batch:
// n_tiles * tw * th x 3 radiance sums of n_samples samples in the render calls' slot order) added onto
// d_io_sum (W x H x 3), folded into the moments state d_io_state (W x H x 4, 16-byte aligned) by
// moments_kernel's update for one frame, and the n_tiles x 4 words of d_records (zeroed on the stream first)
// filled with each tile's in-frame pixels, pixels over the target, bits of the greatest relative standard
// error among the pixels with two batches or more, and pixels with fewer.  tile_ids is a HOST pointer, read
// before the call returns; the caller has validated it: every id inside the ceil(W / tw) x ceil(H / th)
// grid and none twice (two blocks would race on the same pixels), tw and th powers of two with
// tw * th in kMinTilePixels..kMaxTilePixels, n_tiles >= 1 and n_tiles * tw * th < 2^31.  Pixels of tiles not
// listed are neither read nor written.
//
// Finiteness: prt_moments_add's statement holds for the state.  With a finite state the relative standard
// error sqrt(max(var_mean, 0)) / (|mean| + eps_r) is finite and >= +0, so its bits order as the floats do.
hipError_t enqueue_adaptive(const float* d_batch, const int32_t* tile_ids, int n_tiles, int tw, int th, int W, int H,
                            const float* d_feat, const AdaptiveParams& p, float* d_io_sum, float* d_io_state,
                            uint32_t* d_records, hipStream_t stream);

}  // namespace prt_dn

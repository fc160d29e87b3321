// prt_denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
// albedo-demodulated radiance, guided by first-hit normal and depth.
//
// Arithmetic contract: every operation is an IEEE f32 add, mul, div, sqrt, min, max, abs or floor in the
// association written here (the unit is compiled with -ffp-contract=off and correctly rounded
// division / sqrt), so tests/atrous_ref.py and its kin restate it in NumPy bit for bit.  No exp / pow.
//
// Frames are [x][y] with y contiguous (pixel index x * H + y).  One pixel per lane, 64 lanes along
// y: the 16-byte loads of a tap are contiguous over a wave.  Taps come straight from global memory, except in the variance estimate
// of the variance-guided mode, which stages its 7 x 7 windows in LDS.  The sample-moments kernels at the
// end (moments_kernel, var_given_kernel) read and write each pixel once and take no taps;
// adaptive_kernel, which shares moments_kernel's update, is the one kernel with a mapping of its own
// (tile chunks, its batch transposed through LDS); temporal_kernel, the last one, gathers four taps per
// pixel from the previous frame's planes, with or without per-object motion.
#include "prt_denoise.h"

namespace prt_dn {

namespace {

constexpr int kBlockY = 64;   // lanes along y (one wave)
constexpr int kBlockX = 4;    // waves per block, along x
constexpr uint32_t kHit = 1u, kBad = 2u;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ bool pixel_of_lane(int W, int H, int& x, int& y) {
    y = (int)blockIdx.x * kBlockY + (int)threadIdx.x;
    x = (int)blockIdx.y * kBlockX + (int)threadIdx.y;
    return x < W && y < H;
}

// ---- the per-pixel prologue and epilogue, shared by pre_kernel, moments_kernel, temporal_kernel and post_kernel ----
struct Rgb {
    float r, g, b;
};

__device__ __forceinline__ Rgb load_rgb(const float* c) { return {c[0], c[1], c[2]}; }

__device__ __forceinline__ void store_rgb(float* o, const Rgb& c) {
    o[0] = c.r;
    o[1] = c.g;
    o[2] = c.b;
}

// the albedo of the features `f` with its floor: what the demodulation divides by
__device__ __forceinline__ Rgb albedo_floor(const float* f, float eps_a) {
    return {fmaxf(f[0], eps_a), fmaxf(f[1], eps_a), fmaxf(f[2], eps_a)};
}

__device__ __forceinline__ Rgb demodulate(const Rgb& c, const Rgb& a) { return {c.r / a.r, c.g / a.g, c.b / a.b}; }

__device__ __forceinline__ Rgb remodulate(const Rgb& i, const Rgb& a) { return {i.r * a.r, i.g * a.g, i.b * a.b}; }

// a finite colour over a tiny albedo may overflow: such a pixel is set aside like a non-finite one,
// and so is a pixel with a non-finite feature (its weights, as a tap or a centre, would be NaN)
__device__ __forceinline__ bool set_aside(const Rgb& c, const Rgb& i, const float* f) {
    bool bad = !(finite_f(c.r) && finite_f(c.g) && finite_f(c.b) && finite_f(i.r) && finite_f(i.g) && finite_f(i.b));
#pragma unroll
    for (int j = 0; j < 8; ++j) bad = bad || !finite_f(f[j]);
    return bad;
}

// A pixel as the filter and the temporal accumulation take it in: colour c, floored albedo a, the colour i
// demodulated where a surface was hit, and whether the pixel is set aside.
struct Pixel {
    Rgb c, a, i;
    bool hit, bad;
};

__device__ __forceinline__ Pixel prepare(const float* color3, const float* f, float eps_a) {
    Pixel px;
    px.c = load_rgb(color3);
    px.hit = f[7] > 0.0f;
    px.a = albedo_floor(f, eps_a);
    px.i = px.hit ? demodulate(px.c, px.a) : px.c;
    px.bad = set_aside(px.c, px.i, f);
    return px;
}

// pre-pass: demodulate, normalise the normal, depth gradient, classify, repack
__global__ __launch_bounds__(kBlockX* kBlockY) void pre_kernel(const float* __restrict__ color,
                                                               const float* __restrict__ feat, int W, int H,
                                                               float eps_a, float4* __restrict__ iz,
                                                               float4* __restrict__ nc, float2* __restrict__ grad) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float* f = feat + p * 8;
    const Pixel px = prepare(color + p * 3, f, eps_a);
    const float nx = f[3], ny = f[4], nz = f[5];
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (len > 0.0f) {
        ux = nx / len;
        uy = ny / len;
        uz = nz / len;
    }
    const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1;
    const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
    // a difference that reaches a neighbour's non-finite depth counts as no gradient
    float gx = 0.5f * (feat[((size_t)xp * H + y) * 8 + 6] - feat[((size_t)xm * H + y) * 8 + 6]);
    float gy = 0.5f * (feat[((size_t)x * H + yp) * 8 + 6] - feat[((size_t)x * H + ym) * 8 + 6]);
    if (!finite_f(gx)) gx = 0.0f;
    if (!finite_f(gy)) gy = 0.0f;
    iz[p] = make_float4(px.i.r, px.i.g, px.i.b, f[6]);
    nc[p] = make_float4(ux, uy, uz, __uint_as_float((px.hit ? kHit : 0u) | (px.bad ? kBad : 0u)));
    grad[p] = make_float2(gx, gy);
}

// e(x) = (1 / (1 + x / 16))^16 by four squarings: the reproducible stand-in for exp(-x)
__device__ __forceinline__ float e16(float x) {
    float r = 1.0f / (1.0f + x * 0.0625f);
    r = r * r;
    r = r * r;
    r = r * r;
    return r * r;
}

// power-128 normal weight
__device__ __forceinline__ float normal_weight(const float4& np, const float4& nq) {
    float wn = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
#pragma unroll
    for (int j = 0; j < 7; ++j) wn = wn * wn;
    return wn;
}

// depth weight of a tap at pixel offset (ox, oy): the depth difference against the centre's depth gradient
__device__ __forceinline__ float depth_weight(float zp, float zq, const float2& g, float ox, float oy, float sigma_z,
                                              float eps_z) {
    const float gd = g.x * ox + g.y * oy;
    return e16(fabsf(zp - zq) / (sigma_z * fabsf(gd) + eps_z));
}

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// One a-trous pass at `step`.  Fixed filter (kVar false): src is (I.rgb, Z), the colour term is the squared
// colour distance over sigma = (sigma_c * 2^-i)^2; zp and eps_l are not read.  Variance-guided (kVar true; the
// spatial half of SVGF, Schied et al. 2017): src is (I.rgb, var) with the depth in the plane zp, the colour
// term is the luminance distance over sigma = sigma_l times the 3 x 3-prefiltered standard deviation, and
// the variance is carried along.  tests/atrous_ref.py and tests/atrous_var_ref.py restate the two.
template <bool kVar>
__global__ __launch_bounds__(kBlockX* kBlockY) void pass_kernel(const float4* __restrict__ src,
                                                                float4* __restrict__ dst,
                                                                const float4* __restrict__ nc,
                                                                const float2* __restrict__ grad,
                                                                const float* __restrict__ zp, int W, int H, int step,
                                                                float sigma, float sigma_z, float eps_z, float eps_l) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float4 ip = src[p];
    const float4 np = nc[p];
    const uint32_t cls = __float_as_uint(np.w);
    // a non-finite pixel and a miss (no surface: its normal is 0, so no tap but its own has weight) keep their value
    if (cls != kHit) {
        dst[p] = ip;
        return;
    }
    float den = sigma, lp = 0.0f, zc = ip.w;
    if constexpr (kVar) {
        const float gk[3] = {0.25f, 0.125f, 0.0625f};
        float gv = 0.0f, gs = 0.0f;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= H) continue;
                const size_t q = (size_t)qx * (size_t)H + (size_t)qy;
                if (__float_as_uint(nc[q].w) != cls) continue;
                const float gq = gk[(dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)];
                gv = gv + gq * src[q].w;
                gs = gs + gq;
            }
        }
        const float sd = sqrtf(gv / gs);
        den = sigma * sd + eps_l;
        lp = lum(ip.x, ip.y, ip.z);
        zc = zp[p];
    }
    const float2 g = grad[p];
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sum_w = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + step * dx;
        if (qx < 0 || qx >= W) continue;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + step * dy;
            if (qy < 0 || qy >= H) continue;
            const size_t q = (size_t)qx * (size_t)H + (size_t)qy;
            const float4 nq = nc[q];
            if (__float_as_uint(nq.w) != cls) continue;   // bad_q, or hit_q != hit_p
            const float4 iq = src[q];
            const float h = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
            float w = h;
            if (dx != 0 || dy != 0) {
                float zq = iq.w;
                if constexpr (kVar) zq = zp[q];
                const float wz = depth_weight(zc, zq, g, (float)(step * dx), (float)(step * dy), sigma_z, eps_z);
                float xc;
                if constexpr (kVar) {
                    xc = fabsf(lp - lum(iq.x, iq.y, iq.z)) / den;
                } else {
                    const float dr = ip.x - iq.x, dg = ip.y - iq.y, db = ip.z - iq.z;
                    xc = ((dr * dr + dg * dg) + db * db) / den;
                }
                w = ((h * normal_weight(np, nq)) * wz) * e16(xc);
            }
            sum_w = sum_w + w;
            s0 = s0 + w * iq.x;
            s1 = s1 + w * iq.y;
            s2 = s2 + w * iq.z;
            if constexpr (kVar) sv = sv + (w * w) * iq.w;
        }
    }
    float last = ip.w;   // the fixed filter carries the depth
    if constexpr (kVar) {
        last = sv / (sum_w * sum_w);
        if (!finite_f(last)) last = 0.0f;
    }
    dst[p] = make_float4(s0 / sum_w, s1 / sum_w, s2 / sum_w, last);
}

// post-pass: re-modulate; a set-aside pixel returns its input colour
__global__ __launch_bounds__(kBlockX* kBlockY) void post_kernel(const float4* __restrict__ iz,
                                                                const float4* __restrict__ nc,
                                                                const float* __restrict__ color,
                                                                const float* __restrict__ feat, int W, int H,
                                                                float eps_a, float* __restrict__ out) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const uint32_t cls = __float_as_uint(nc[p].w);
    Rgb o;
    if (cls & kBad) {
        o = load_rgb(color + p * 3);
    } else {
        const float4 i = iz[p];
        o = {i.x, i.y, i.z};
        if (cls & kHit) o = remodulate(o, albedo_floor(feat + p * 8, eps_a));
    }
    store_rgb(out + p * 3, o);
}

// ---- variance-guided mode ----
// The pre-pass, the passes and the post-pass are the ones above.  Between pre and post the colour travels as
// (I.rgb, var) and the depth in a float plane of its own; tests/atrous_var_ref.py restates the estimate.

// the caller's variance is taken as it is when it is finite and >= 0 (a -0 passes)
__device__ __forceinline__ bool usable_variance(float t) { return finite_f(t) && t >= 0.0f; }

// the tail of both variance steps: (I.rgb, Z) repacked into (I.rgb, var) and the depth plane, and the
// variance actually used into the caller's plane, if there is one
__device__ __forceinline__ void store_repacked(size_t p, const float4& ip, float var, float4* iv, float* zp,
                                               float* out_var) {
    iv[p] = make_float4(ip.x, ip.y, ip.z, var);
    zp[p] = ip.w;
    if (out_var) out_var[p] = var;
}

// variance estimate: per hit pixel the weighted second central moment of the luminance over the
// 7 x 7 window at step 1; repacks (I.rgb, Z) into (I.rgb, var) and the depth plane.  With a plane in_var
// (the mixed mode; null otherwise) a usable pixel whose in_var is a usable variance takes that value in
// place of the estimate, and every other pixel keeps the estimate.  The block's
// 10 x 70 neighbourhood (its 4 x 64 pixels and a 3-pixel halo) is staged in LDS as luminance, depth,
// normal and a "usable" flag (16.8 KB): measured against taps straight from global memory the
// kernel takes 0.66 of the time at 4096^2.
constexpr int kHalo = 3;
constexpr int kTileX = kBlockX + 2 * kHalo, kTileY = kBlockY + 2 * kHalo;

__global__ __launch_bounds__(kBlockX* kBlockY) void var_estimate_kernel(const float4* __restrict__ iz,
                                                                        const float4* __restrict__ nc,
                                                                        const float2* __restrict__ grad,
                                                                        const float* __restrict__ in_var, int W, int H,
                                                                        float sigma_z, float eps_z,
                                                                        float4* __restrict__ iv, float* __restrict__ zp,
                                                                        float* __restrict__ out_var) {
    __shared__ float s_l[kTileX][kTileY], s_z[kTileX][kTileY], s_nx[kTileX][kTileY], s_ny[kTileX][kTileY],
        s_nz[kTileX][kTileY];
    __shared__ uint32_t s_ok[kTileX][kTileY];
    const int x0 = (int)blockIdx.y * kBlockX - kHalo, y0 = (int)blockIdx.x * kBlockY - kHalo;
    for (int e = (int)threadIdx.y * kBlockY + (int)threadIdx.x; e < kTileX * kTileY; e += kBlockX * kBlockY) {
        const int tx = e / kTileY, ty = e - tx * kTileY;
        const int qx = x0 + tx, qy = y0 + ty;
        float l = 0.0f, z = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f;
        uint32_t ok = 0u;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const size_t q = (size_t)qx * (size_t)H + (size_t)qy;
            const float4 nq = nc[q];
            const float4 iq = iz[q];
            ok = __float_as_uint(nq.w) == kHit ? 1u : 0u;
            l = lum(iq.x, iq.y, iq.z);
            z = iq.w;
            nx = nq.x;
            ny = nq.y;
            nz = nq.z;
        }
        s_l[tx][ty] = l;
        s_z[tx][ty] = z;
        s_nx[tx][ty] = nx;
        s_ny[tx][ty] = ny;
        s_nz[tx][ty] = nz;
        s_ok[tx][ty] = ok;
    }
    __syncthreads();
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float4 ip = iz[p];
    const float4 np = nc[p];
    const int cx = (int)threadIdx.y + kHalo, cy = (int)threadIdx.x + kHalo;
    float var = 0.0f;
    if (__float_as_uint(np.w) == kHit) {
        const float2 g = grad[p];
        float sw = 0.0f, m1 = 0.0f, m2 = 0.0f;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
#pragma unroll
            for (int dy = -3; dy <= 3; ++dy) {
                if (!s_ok[cx + dx][cy + dy]) continue;   // outside the frame, or not a usable tap
                float w = 1.0f;
                if (dx != 0 || dy != 0) {
                    const float4 nq = make_float4(s_nx[cx + dx][cy + dy], s_ny[cx + dx][cy + dy], s_nz[cx + dx][cy + dy], 0.0f);
                    w = normal_weight(np, nq) *
                        depth_weight(ip.w, s_z[cx + dx][cy + dy], g, (float)dx, (float)dy, sigma_z, eps_z);
                }
                const float l = s_l[cx + dx][cy + dy];
                sw = sw + w;
                m1 = m1 + w * l;
                m2 = m2 + w * (l * l);
            }
        }
        const float mu = m1 / sw;
        var = fmaxf(0.0f, m2 / sw - mu * mu);
        if (!finite_f(var)) var = 0.0f;
        if (in_var) {
            const float t = in_var[p];
            if (usable_variance(t)) var = t;
        }
    }
    store_repacked(p, ip, var, iv, zp, out_var);
}

// ---- variance from per-pixel sample moments (tests/moments_ref.py restates both) ----

// given variance: stands where var_estimate_kernel stands.  Repacks (I.rgb, Z) into (I.rgb, v) and the
// depth plane, with v the caller's variance at a usable pixel when it is a usable variance, else 0.
__global__ __launch_bounds__(kBlockX* kBlockY) void var_given_kernel(const float4* __restrict__ iz,
                                                                     const float4* __restrict__ nc,
                                                                     const float* __restrict__ in_var, int W, int H,
                                                                     float4* __restrict__ iv, float* __restrict__ zp,
                                                                     float* __restrict__ out_var) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float4 ip = iz[p];
    float var = 0.0f;
    if (__float_as_uint(nc[p].w) == kHit) {
        const float t = in_var[p];
        if (usable_variance(t)) var = t;
    }
    store_repacked(p, ip, var, iv, zp, out_var);
}

// ---- the moments update, shared by moments_kernel and adaptive_kernel ----

// the demodulated luminance of the mean of a batch of n samples with the radiance sums S
__device__ __forceinline__ float batch_luminance(const Rgb& S, float n, bool hit, const Rgb& a) {
    Rgb i = {S.r / n, S.g / n, S.b / n};
    if (hit) i = demodulate(i, a);
    return lum(i.r, i.g, i.b);
}

// Welford's update with one batch luminance; one that is not finite is skipped
__device__ __forceinline__ void welford_add(float& k, float& mean, float& m2, float l) {
    if (!finite_f(l)) return;
    k = k + 1.0f;
    const float d = l - mean;
    mean = mean + d / k;
    m2 = m2 + d * (l - mean);
}

// the closing step: the variance of the mean over the k batches seen, 0 below two and where it is not finite
__device__ __forceinline__ float variance_of_mean(float k, float m2) {
    float vm = 0.0f;
    if (k >= 2.0f) vm = (m2 / (k - 1.0f)) / k;
    if (!finite_f(vm)) vm = 0.0f;
    return vm;
}

// running Welford update of the demodulated luminance of the batch means over n_frames frames of
// radiance sums; state (k, mean, M2, var_mean) per pixel, one 16-byte load and store
__global__ __launch_bounds__(kBlockX* kBlockY) void moments_kernel(const float* __restrict__ sums, int n_frames,
                                                                   size_t frame_pitch, float n,
                                                                   const float* __restrict__ feat, int W, int H,
                                                                   float eps_a, float4* __restrict__ state) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float* f = feat + p * 8;
    const bool hit = f[7] > 0.0f;
    const Rgb a = albedo_floor(f, eps_a);
    const float4 s = state[p];
    float k = s.x, mean = s.y, m2 = s.z;
    for (int fr = 0; fr < n_frames; ++fr)
        welford_add(k, mean, m2, batch_luminance(load_rgb(sums + (size_t)fr * frame_pitch + p * 3), n, hit, a));
    state[p] = make_float4(k, mean, m2, variance_of_mean(k, m2));
}

// ---- adaptive sampling (tests/adaptive_ref.py restates it) ----
// One batch of a list of tiles folded into the frame's sums and moments, and every listed tile scored
// against the noise target.  The batch comes in the render calls' slot order (tile-major, then row ly, then
// column lx: x-contiguous), the frame planes are [x][y] (y-contiguous): a block takes one chunk of one
// tile, kChunk pixels as cx x cy, reads the chunk's rows of the batch along x (coalesced) into LDS, and
// turns to lanes along y for the planes, cy pixels (16 B of state each) contiguous per column.  The rows
// are padded by one float, so the transposed read has an odd stride.
//
// The tile ids travel in the kernel arguments, kTilesPerLaunch to a launch: the unit keeps no device
// buffer of its own and enqueues no copy from host memory that would have to outlive the call.
constexpr int kChunk = 256;             // pixels of a chunk, threads of a block
constexpr int kChunkFloats = 1024;      // the most a chunk's padded rows take: cx = 1, cy = 256
constexpr int kTilesPerLaunch = 896;    // 3584 of the 4096 bytes of kernel arguments

struct TileIds {
    int32_t id[kTilesPerLaunch];
};

// the shapes of tile and chunk as shifts, and the frame
struct AdaptiveShape {
    int W, H, tiles_x, log_tw, log_th, log_cx, log_cy;
};

__global__ __launch_bounds__(kChunk) void adaptive_kernel(const float* __restrict__ batch, const TileIds ids,
                                                          int first_tile, const AdaptiveShape g,
                                                          const float* __restrict__ feat, const AdaptiveParams P,
                                                          float* __restrict__ io_sum, float4* __restrict__ io_state,
                                                          uint32_t* __restrict__ records) {
    __shared__ float s_batch[kChunkFloats];
    __shared__ uint32_t s_rec[4];
    const int tid = (int)threadIdx.x;
    const int log_nx = g.log_tw - g.log_cx, log_chunks = log_nx + (g.log_th - g.log_cy);
    const int tile = (int)(blockIdx.x >> log_chunks), chunk = (int)(blockIdx.x & ((1u << log_chunks) - 1u));
    const int id = ids.id[tile];
    // the chunk's origin in the tile and in the frame
    const int lx0 = (chunk & ((1 << log_nx) - 1)) << g.log_cx, ly0 = (chunk >> log_nx) << g.log_cy;
    const int x0 = ((id % g.tiles_x) << g.log_tw) + lx0, y0 = ((id / g.tiles_x) << g.log_th) + ly0;
    if (x0 >= g.W || y0 >= g.H) return;   // the whole chunk lies outside the frame (the whole block returns)
    if (tid < 4) s_rec[tid] = 0u;

    // 1. the chunk's rows of the batch, lanes along x; slots outside the frame are not read
    const int row_floats = 3 << g.log_cx, pitch = row_floats + 1;
    const size_t slot0 = ((size_t)(first_tile + tile) << (g.log_tw + g.log_th)) + ((size_t)ly0 << g.log_tw) + (size_t)lx0;
    for (int i = tid; i < (row_floats << g.log_cy); i += kChunk) {
        const int row = (i >> g.log_cx) / 3, col = i - row * row_floats;
        if (x0 + col / 3 < g.W && y0 + row < g.H)
            s_batch[row * pitch + col] = batch[(slot0 + ((size_t)row << g.log_tw)) * 3 + (size_t)col];
    }
    __syncthreads();

    // 2. the pixel of this lane, lanes along y
    const int lx = tid >> g.log_cy, ly = tid & ((1 << g.log_cy) - 1);
    const int x = x0 + lx, y = y0 + ly;
    const bool in = tid < (1 << (g.log_cx + g.log_cy)) && x < g.W && y < g.H;
    bool young = false, over = false;
    uint32_t e_bits = 0u;
    if (in) {
        const size_t p = (size_t)x * (size_t)g.H + (size_t)y;
        const float* sb = s_batch + ly * pitch + lx * 3;
        const Rgb S = load_rgb(sb);
        const Rgb sum = load_rgb(io_sum + p * 3);
        store_rgb(io_sum + p * 3, {sum.r + S.r, sum.g + S.g, sum.b + S.b});
        const float* f = feat + p * 8;
        const bool hit = f[7] > 0.0f;
        const Rgb a = albedo_floor(f, P.eps_a);
        const float4 s = io_state[p];
        float k = s.x, mean = s.y, m2 = s.z;
        welford_add(k, mean, m2, batch_luminance(S, P.n_samples, hit, a));
        const float vm = variance_of_mean(k, m2);
        io_state[p] = make_float4(k, mean, m2, vm);
        // 3. the relative standard error; fmaxf(vm, 0) with the zero's sign settled: a -0 counts as +0
        const float e = sqrtf(vm > 0.0f ? vm : 0.0f) / (fabsf(mean) + P.eps_r);
        young = k < 2.0f;
        over = young || e > P.target;
        if (!young) e_bits = __float_as_uint(e);
    }

    // 4. the tile's record: counts by ballot, the maximum of the non-negative floats as an integer maximum of
    //    their bits; one LDS atomic per wave, one global atomic per block and word
    const unsigned long long m_in = __ballot(in), m_over = __ballot(over), m_young = __ballot(young);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)e_bits, off);
        e_bits = o > e_bits ? o : e_bits;
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_rec[0], (uint32_t)__popcll(m_in));
        atomicAdd(&s_rec[1], (uint32_t)__popcll(m_over));
        atomicMax(&s_rec[2], e_bits);
        atomicAdd(&s_rec[3], (uint32_t)__popcll(m_young));
    }
    __syncthreads();
    if (tid < 4) {
        uint32_t* r = records + (size_t)(first_tile + tile) * 4 + tid;
        const uint32_t v = s_rec[tid];
        if (tid == 2) atomicMax(r, v);
        else atomicAdd(r, v);
    }
}

// ---- temporal accumulation (DESIGN.md §11 "Temporal accumulation" and "Moving objects"; tests/temporal_ref.py
// restates both instantiations, the one with per-object motion as its `ids` clauses) ----
// The previous frame's integrated demodulated colour and luminance moments, reprojected through the first-hit
// features into this frame's camera (the temporal half of SVGF, Schied et al. 2017).  The state is two float4
// per pixel: (I.rgb, h) and (m1, m2, var, 0).  The four bilinear taps of a pixel come straight from global
// memory: neighbouring lanes reproject to neighbouring previous pixels, so a wave's taps share cache lines.
// The pinhole ray of PackedCamera.gen_ray is restated here at the pixel centre; floor joins the operations of
// the arithmetic contract.

constexpr uint32_t kNoVariance = 0x7fc00000u;   // the quiet NaN that marks "no trustworthy temporal variance"

// the parts of the two 24-float camera records the kernel reads, by value in the kernel arguments
struct Cameras {
    float cur[12];    // rows 0..2 of this frame's record: (side_i, up_i, back_i, eye_i) per world axis i
    float sw, sh, fd;
    float prev[12];
    float psw, psh, pfd;
};

// kMotion false is the static world: `mo` is not read and every pixel goes the way `cams_equal` says.  kMotion
// true carries the first hit of a pixel whose object id has a row into the previous frame's world before it is
// projected, turns its normal along, and asks every tap for the same id (SVGF's mesh-id test); the one-tap
// shortcut of equal cameras is then decided per pixel.
template <bool kMotion>
__global__ __launch_bounds__(kBlockX* kBlockY) void temporal_kernel(
    const float* __restrict__ color, const float* __restrict__ feat, const float* __restrict__ prev_feat,
    const float4* __restrict__ prev_state, const Cameras cams, int W, int H, int cams_equal, const TemporalParams P,
    const Motion mo, float4* __restrict__ state, float* __restrict__ out_color, float* __restrict__ out_var) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float marker = __uint_as_float(kNoVariance);

    // 1. prepare: the filter's demodulation and its notion of a pixel that takes no part
    float F[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) F[j] = feat[p * 8 + j];
    const Pixel px = prepare(color + p * 3, F, P.eps_a);
    const bool hit = px.hit;
    const float i0 = px.i.r, i1 = px.i.g, i2 = px.i.b;
    if (px.bad) {
        state[p * 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        state[p * 2 + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (out_color) store_rgb(out_color + p * 3, px.c);
        if (out_var) out_var[p] = marker;
        return;
    }
    const float l = lum(i0, i1, i2);

    // 2. without history: the state a miss, the first frame and every rejected reprojection end in
    float n0 = i0, n1 = i1, n2 = i2, nh = 1.0f, nm1 = l, nm2 = l * l, nv = marker;

    // the object's row: none for an id outside the table (the static path), "no previous pose" when an entry is
    // not finite, and the one-tap shortcut only while it is bytewise the identity
    bool is_static = cams_equal != 0, has_row = false, no_pose = false;
    int id = 0;
    float M[12];
    if constexpr (kMotion) {
        id = mo.ids[p];
        if (hit && prev_state && id >= 0 && id < mo.n_objects) {
            const float* row = mo.rows + (size_t)id * 12;
            bool identity = true;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                M[j] = row[j];
                no_pose = no_pose || !finite_f(M[j]);
                identity = identity && __float_as_uint(M[j]) == (j % 5 == 0 ? 0x3f800000u : 0u);
            }
            has_row = true;
            is_static = is_static && identity;
        }
    }

    if (hit && prev_state && !no_pose) {
        // 3. project the first hit into the previous camera
        float Np[3] = {F[3], F[4], F[5]};
        float r = F[6], px = (float)x, py = (float)y;
        bool in_range = true;
        if (!is_static) {
            const float u = ((float)x + 0.5f) / (float)(W - 1), v = ((float)y + 0.5f) / (float)(H - 1);
            const float rx = (u - 0.5f) * cams.sw / 0.5f, ry = (v - 0.5f) * cams.sh / 0.5f, rz = -cams.fd;
            float E[3], f[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float* c = cams.cur + 4 * i;
                E[i] = c[3];
                f[i] = (((rx * c[0] + ry * c[1]) + rz * c[2]) + c[3]) - E[i];
            }
            const float ln = sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
            float X[3], rel[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) X[i] = E[i] + F[6] * (f[i] / ln);
            if constexpr (kMotion) {
                if (has_row) {
                    // this frame's world position and normal in the previous frame's world
                    float Xp[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float* m = M + 4 * i;
                        Xp[i] = ((m[0] * X[0] + m[1] * X[1]) + m[2] * X[2]) + m[3];
                        Np[i] = (m[0] * F[3] + m[1] * F[4]) + m[2] * F[5];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) X[i] = Xp[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) rel[i] = X[i] - cams.prev[4 * i + 3];
            r = sqrtf((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2]);
            const float a = (rel[0] * cams.prev[0] + rel[1] * cams.prev[4]) + rel[2] * cams.prev[8];
            const float b = (rel[0] * cams.prev[1] + rel[1] * cams.prev[5]) + rel[2] * cams.prev[9];
            const float c = (rel[0] * cams.prev[2] + rel[1] * cams.prev[6]) + rel[2] * cams.prev[10];
            const float nc = -c;
            px = (0.5f + ((0.5f * cams.pfd) * a) / (cams.psw * nc)) * (float)(W - 1) - 0.5f;
            py = (0.5f + ((0.5f * cams.pfd) * b) / (cams.psh * nc)) * (float)(H - 1) - 0.5f;
            // 4. the range test, in float comparisons a NaN fails, before any conversion or load
            in_range = c < 0.0f && px > -1.0f && px < (float)W && py > -1.0f && py < (float)H;
        }
        if (in_range) {
            int tx[2] = {x, x}, ty[2] = {y, y};
            float wx[2] = {1.0f, 0.0f}, wy[2] = {1.0f, 0.0f};
            if (!is_static) {
                const float fx0 = floorf(px), fy0 = floorf(py);
                const float fx = px - fx0, fy = py - fy0;
                tx[0] = (int)fx0;
                tx[1] = tx[0] + 1;
                ty[0] = (int)fy0;
                ty[1] = ty[0] + 1;
                wx[0] = 1.0f - fx;
                wx[1] = fx;
                wy[0] = 1.0f - fy;
                wy[1] = fy;
            }
            // 5. the taps, x outer, y inner; a static camera takes the one tap q = p with weight 1
            float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sh = 0.0f, sm1 = 0.0f, sm2 = 0.0f;
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) {
                const int qx = tx[jx];
                if (qx < 0 || qx >= W) continue;
#pragma unroll
                for (int jy = 0; jy < 2; ++jy) {
                    const int qy = ty[jy];
                    if (qy < 0 || qy >= H || (is_static && (jx | jy))) continue;
                    const size_t q = (size_t)qx * (size_t)H + (size_t)qy;
                    if constexpr (kMotion) {
                        if (mo.prev_ids[q] != id) continue;   // another object stood there
                    }
                    const float4 h0 = prev_state[q * 2];
                    if (!(h0.w > 0.0f)) continue;
                    const float* G = prev_feat + q * 8;
                    if (!(G[7] > 0.0f)) continue;
                    const float nd = (Np[0] * G[3] + Np[1] * G[4]) + Np[2] * G[5];
                    if (!(nd >= P.tau_n)) continue;
                    if (!(fabsf(G[6] - r) <= P.tau_z * r)) continue;
                    const float da = fmaxf(fmaxf(fabsf(G[0] - F[0]), fabsf(G[1] - F[1])), fabsf(G[2] - F[2]));
                    if (!(da <= P.tau_a)) continue;
                    const float4 h1 = prev_state[q * 2 + 1];
                    const float w = wx[jx] * wy[jy];
                    sw = sw + w;
                    s0 = s0 + w * h0.x;
                    s1 = s1 + w * h0.y;
                    s2 = s2 + w * h0.z;
                    sh = sh + w * h0.w;
                    sm1 = sm1 + w * h1.x;
                    sm2 = sm2 + w * h1.y;
                }
            }
            // 6. valid history and blend
            if (sw >= P.w_min) {
                const float g0 = s0 / sw, g1 = s1 / sw, g2 = s2 / sw, gm1 = sm1 / sw, gm2 = sm2 / sw;
                nh = sh / sw + 1.0f;
                const float ac = fmaxf(1.0f / nh, P.alpha), am = fmaxf(1.0f / nh, P.alpha_m);
                n0 = g0 + ac * (i0 - g0);
                n1 = g1 + ac * (i1 - g1);
                n2 = g2 + ac * (i2 - g2);
                nm1 = gm1 + am * (l - gm1);
                nm2 = gm2 + am * (l * l - gm2);
                // 7. the variance of the integrated luminance, once the history is long enough
                if (nh >= P.min_history) nv = fmaxf(0.0f, nm2 - nm1 * nm1) * ac;
            }
        }
    }
    state[p * 2] = make_float4(n0, n1, n2, nh);
    state[p * 2 + 1] = make_float4(nm1, nm2, nv, 0.0f);
    if (out_color) {
        const Rgb n = {n0, n1, n2};
        store_rgb(out_color + p * 3, hit ? remodulate(n, px.a) : n);
    }
    if (out_var) out_var[p] = nv;
}

// the planes of a frame's scratch, in the order work_bytes counts them
struct Planes {
    float4* a[2];   // ping-pong (I.rgb, Z) or (I.rgb, var)
    float4* nc;     // (N.xyz, class)
    float2* grad;   // depth gradient
    float* zp;      // depth; only the variance-guided modes' scratch holds it
    Planes(void* d_work, int W, int H, bool variance) {
        const size_t n = (size_t)W * (size_t)H;
        a[0] = static_cast<float4*>(d_work);
        a[1] = a[0] + n;
        nc = a[1] + n;
        grad = reinterpret_cast<float2*>(nc + n);
        zp = variance ? reinterpret_cast<float*>(grad + n) : nullptr;
    }
};

// One kernel over the W x H frame on `stream`.  An error left on this thread by earlier, unrelated calls
// is not ours: it is cleared before the launch, and the launch's own is returned.
template <typename... Params, typename... Args>
hipError_t launch(void (*kernel)(Params...), int W, int H, hipStream_t stream, Args... args) {
    const dim3 grid((unsigned)((H + kBlockY - 1) / kBlockY), (unsigned)((W + kBlockX - 1) / kBlockX));
    (void)hipGetLastError();
    kernel<<<grid, dim3(kBlockY, kBlockX), 0, stream>>>(args...);
    return hipGetLastError();
}

// `iterations` passes from s.a[0] and the post-pass; p.sigma is sigma_c (fixed) or sigma_l (variance-guided)
template <bool kVar>
hipError_t passes_and_post(const Planes& s, const float* d_color, const float* d_feat, int W, int H, int iterations,
                           const FilterParams& p, float* d_out, hipStream_t stream) {
    int cur = 0;
    for (int i = 0; i < iterations; ++i) {
        float sg = p.sigma;
        if constexpr (!kVar) {
            // sigma_c * 2^-i is an exact scaling; its square is one f32 multiplication
            const float sc = p.sigma * (1.0f / (float)(1 << i));
            sg = sc * sc;
        }
        const hipError_t e = launch(pass_kernel<kVar>, W, H, stream, s.a[cur], s.a[cur ^ 1], s.nc, s.grad, s.zp, W, H,
                                    1 << i, sg, p.sigma_z, p.eps_z, p.eps_l);
        if (e != hipSuccess) return e;
        cur ^= 1;
    }
    return launch(post_kernel, W, H, stream, s.a[cur], s.nc, d_color, d_feat, W, H, p.eps_a, d_out);
}

}  // namespace

size_t work_bytes(int W, int H, bool variance) {
    const size_t n = (size_t)W * (size_t)H;
    return (n * (variance ? 60 : 56) + 255) & ~(size_t)255;
}

hipError_t enqueue_filter(Mode mode, const float* d_color, const float* d_feat, const float* d_in_var, int W, int H,
                          int iterations, const FilterParams& p, float* d_out, float* d_out_var, void* d_work,
                          hipStream_t stream) {
    const bool variance = mode != Mode::kFixed;
    const Planes s(d_work, W, H, variance);
    // The fixed filter's pre-pass writes (I.rgb, Z) where the passes start.  In the variance-guided modes it
    // writes into the second ping-pong plane, and the variance step repacks that into the first.
    hipError_t e = launch(pre_kernel, W, H, stream, d_color, d_feat, W, H, p.eps_a, s.a[variance ? 1 : 0], s.nc, s.grad);
    if (e != hipSuccess) return e;
    if (!variance) return passes_and_post<false>(s, d_color, d_feat, W, H, iterations, p, d_out, stream);
    if (mode == Mode::kGiven)
        e = launch(var_given_kernel, W, H, stream, s.a[1], s.nc, d_in_var, W, H, s.a[0], s.zp, d_out_var);
    else
        e = launch(var_estimate_kernel, W, H, stream, s.a[1], s.nc, s.grad, mode == Mode::kMixed ? d_in_var : nullptr, W,
                   H, p.sigma_z, p.eps_z, s.a[0], s.zp, d_out_var);
    if (e != hipSuccess) return e;
    return passes_and_post<true>(s, d_color, d_feat, W, H, iterations, p, d_out, stream);
}

hipError_t enqueue_moments(const float* d_sums, int n_frames, size_t frame_pitch, float n_samples, const float* d_feat,
                           float eps_a, int W, int H, float* d_io_state, hipStream_t stream) {
    return launch(moments_kernel, W, H, stream, d_sums, n_frames, frame_pitch, n_samples, d_feat, W, H, eps_a,
                  reinterpret_cast<float4*>(d_io_state));
}

hipError_t enqueue_adaptive(const float* d_batch, const int32_t* tile_ids, int n_tiles, int tw, int th, int W, int H,
                            const float* d_feat, const AdaptiveParams& p, float* d_io_sum, float* d_io_state,
                            uint32_t* d_records, hipStream_t stream) {
    AdaptiveShape g = {};
    g.W = W;
    g.H = H;
    g.tiles_x = (W + tw - 1) / tw;
    g.log_tw = __builtin_ctz((unsigned)tw);
    g.log_th = __builtin_ctz((unsigned)th);
    // the chunk: up to 16 pixels along x and the rest of the kChunk along y, widened along x where the tile is flat
    const int log_chunk = __builtin_ctz((unsigned)kChunk);
    g.log_cx = g.log_tw < 4 ? g.log_tw : 4;
    g.log_cy = g.log_th < log_chunk - g.log_cx ? g.log_th : log_chunk - g.log_cx;
    if (g.log_tw < log_chunk - g.log_cy) g.log_cx = g.log_tw;
    else g.log_cx = log_chunk - g.log_cy;
    const int log_chunks = (g.log_tw - g.log_cx) + (g.log_th - g.log_cy);
    (void)hipGetLastError();
    hipError_t e = hipMemsetAsync(d_records, 0, (size_t)n_tiles * 4 * sizeof(uint32_t), stream);
    TileIds ids;
    for (int first = 0; first < n_tiles && e == hipSuccess; first += kTilesPerLaunch) {
        const int n = n_tiles - first < kTilesPerLaunch ? n_tiles - first : kTilesPerLaunch;
        for (int i = 0; i < kTilesPerLaunch; ++i) ids.id[i] = i < n ? tile_ids[first + i] : 0;
        adaptive_kernel<<<dim3((unsigned)n << log_chunks), dim3(kChunk), 0, stream>>>(
            d_batch, ids, first, g, d_feat, p, d_io_sum, reinterpret_cast<float4*>(d_io_state), d_records);
        e = hipGetLastError();
    }
    return e;
}

namespace {

Cameras camera_parts(const float* cam24, const float* prev_cam24) {
    Cameras cams = {};
    for (int i = 0; i < 12; ++i) cams.cur[i] = cam24[i];
    cams.sw = cam24[16];
    cams.sh = cam24[17];
    cams.fd = cam24[18];
    if (prev_cam24) {
        for (int i = 0; i < 12; ++i) cams.prev[i] = prev_cam24[i];
        cams.psw = prev_cam24[16];
        cams.psh = prev_cam24[17];
        cams.pfd = prev_cam24[18];
    }
    return cams;
}

}  // namespace

hipError_t enqueue_temporal(const float* d_color, const float* d_feat, const float* cam24, const float* d_prev_feat,
                            const float* prev_cam24, const float* d_prev_state, const Motion* motion, int W, int H,
                            bool cameras_equal, const TemporalParams& p, float* d_state, float* d_out_color,
                            float* d_out_var, hipStream_t stream) {
    Motion mo = {nullptr, nullptr, nullptr, 0};
    if (motion) {
        mo = *motion;
        if (mo.n_objects == 0) mo.rows = nullptr;   // no rows, no table: whatever the caller's pointer held
    }
    return launch(!motion ? temporal_kernel<false> : temporal_kernel<true>, W, H, stream, d_color, d_feat, d_prev_feat,
                  reinterpret_cast<const float4*>(d_prev_state), camera_parts(cam24, prev_cam24), W, H,
                  cameras_equal ? 1 : 0, p, mo, reinterpret_cast<float4*>(d_state), d_out_color, d_out_var);
}

}  // namespace prt_dn

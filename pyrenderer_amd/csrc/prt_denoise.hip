// prt_denoise.hip — edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on
// albedo-demodulated radiance, guided by first-hit normal and depth.
//
// Arithmetic contract: every operation is an IEEE f32 add, mul, div, sqrt, min, max or abs in the
// association written here (the unit is compiled with -ffp-contract=off and correctly rounded
// division / sqrt), so tests/atrous_ref.py restates it in NumPy bit for bit.  No exp / pow.
//
// Frames are [x][y] with y contiguous (pixel index x * H + y).  One pixel per lane, 64 lanes along
// y: the 16-byte loads of a tap are contiguous over a wave.  Taps come straight from global memory.
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

// pre-pass: demodulate, normalise the normal, depth gradient, classify, repack
__global__ __launch_bounds__(kBlockX* kBlockY) void pre_kernel(const float* __restrict__ color,
                                                               const float* __restrict__ feat, int W, int H,
                                                               float eps_a, float4* __restrict__ iz,
                                                               float4* __restrict__ nc, float2* __restrict__ grad) {
    int x, y;
    if (!pixel_of_lane(W, H, x, y)) return;
    const size_t p = (size_t)x * (size_t)H + (size_t)y;
    const float* f = feat + p * 8;
    const float c0 = color[p * 3], c1 = color[p * 3 + 1], c2 = color[p * 3 + 2];
    const bool hit = f[7] > 0.0f;
    float i0 = c0, i1 = c1, i2 = c2;
    if (hit) {
        i0 = c0 / fmaxf(f[0], eps_a);
        i1 = c1 / fmaxf(f[1], eps_a);
        i2 = c2 / fmaxf(f[2], eps_a);
    }
    // a finite colour over a tiny albedo may overflow: such a pixel is set aside like a non-finite one,
    // and so is a pixel with a non-finite feature (its weights, as a tap or a centre, would be NaN)
    bool bad = !(finite_f(c0) && finite_f(c1) && finite_f(c2) && finite_f(i0) && finite_f(i1) && finite_f(i2));
#pragma unroll
    for (int j = 0; j < 8; ++j) bad = bad || !finite_f(f[j]);
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
    iz[p] = make_float4(i0, i1, i2, f[6]);
    nc[p] = make_float4(ux, uy, uz, __uint_as_float((hit ? kHit : 0u) | (bad ? kBad : 0u)));
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

// one a-trous pass at `step`; sc2 = (sigma_c * 2^-i)^2
__global__ __launch_bounds__(kBlockX* kBlockY) void atrous_kernel(const float4* __restrict__ src,
                                                                  float4* __restrict__ dst,
                                                                  const float4* __restrict__ nc,
                                                                  const float2* __restrict__ grad, int W, int H,
                                                                  int step, float sc2, float sigma_z, float eps_z) {
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
    const float2 g = grad[p];
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sum_w = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
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
                float wn = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
#pragma unroll
                for (int j = 0; j < 7; ++j) wn = wn * wn;
                const float gd = g.x * (float)(step * dx) + g.y * (float)(step * dy);
                const float xz = fabsf(ip.w - iq.w) / (sigma_z * fabsf(gd) + eps_z);
                const float dr = ip.x - iq.x, dg = ip.y - iq.y, db = ip.z - iq.z;
                const float xc = ((dr * dr + dg * dg) + db * db) / sc2;
                w = ((h * wn) * e16(xz)) * e16(xc);
            }
            sum_w = sum_w + w;
            s0 = s0 + w * iq.x;
            s1 = s1 + w * iq.y;
            s2 = s2 + w * iq.z;
        }
    }
    dst[p] = make_float4(s0 / sum_w, s1 / sum_w, s2 / sum_w, ip.w);
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
    float o0, o1, o2;
    if (cls & kBad) {
        o0 = color[p * 3];
        o1 = color[p * 3 + 1];
        o2 = color[p * 3 + 2];
    } else {
        const float4 i = iz[p];
        o0 = i.x;
        o1 = i.y;
        o2 = i.z;
        if (cls & kHit) {
            const float* f = feat + p * 8;
            o0 = o0 * fmaxf(f[0], eps_a);
            o1 = o1 * fmaxf(f[1], eps_a);
            o2 = o2 * fmaxf(f[2], eps_a);
        }
    }
    out[p * 3] = o0;
    out[p * 3 + 1] = o1;
    out[p * 3 + 2] = o2;
}

}  // namespace

size_t work_bytes(int W, int H) {
    const size_t n = (size_t)W * (size_t)H;
    return (n * 56 + 255) & ~(size_t)255;
}

hipError_t enqueue(const float* d_color, const float* d_feat, int W, int H, int iterations, const Params& p,
                   float* d_out, void* d_work, hipStream_t stream) {
    const size_t n = (size_t)W * (size_t)H;
    float4* a[2] = {static_cast<float4*>(d_work), static_cast<float4*>(d_work) + n};
    float4* nc = a[1] + n;
    float2* grad = reinterpret_cast<float2*>(nc + n);
    const dim3 block(kBlockY, kBlockX);
    const dim3 grid((unsigned)((H + kBlockY - 1) / kBlockY), (unsigned)((W + kBlockX - 1) / kBlockX));
    (void)hipGetLastError();   // an error left on this thread by earlier, unrelated calls is not ours
    pre_kernel<<<grid, block, 0, stream>>>(d_color, d_feat, W, H, p.eps_a, a[0], nc, grad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int cur = 0;
    for (int i = 0; i < iterations; ++i) {
        // sigma_c * 2^-i is an exact scaling; its square is one f32 multiplication
        const float sc = p.sigma_c * (1.0f / (float)(1 << i));
        atrous_kernel<<<grid, block, 0, stream>>>(a[cur], a[cur ^ 1], nc, grad, W, H, 1 << i, sc * sc, p.sigma_z,
                                                  p.eps_z);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        cur ^= 1;
    }
    post_kernel<<<grid, block, 0, stream>>>(a[cur], nc, d_color, d_feat, W, H, p.eps_a, d_out);
    return hipGetLastError();
}

}  // namespace prt_dn

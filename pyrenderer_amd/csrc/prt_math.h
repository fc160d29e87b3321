#pragma once
// prt_math.h — vector math, the guarded fast division / reciprocal / sqrt sequences, the RNG and the
// sampling routines of the device code, under the arithmetic contract (prt_device.h).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prt_kernels.h"

namespace prt {
namespace {

constexpr float kInvPi = 0.31830988618379067154f;
constexpr float kPiOver4 = 0.78539816339744830961f;
constexpr float kTMin = 0.00001f;    // core/tracing.py:127
constexpr float kTMax = 99999.9f;    // core/tracing.py:127
constexpr float kGamma = 0x1.000006p+0f;  // f32(1 + 2*GAMMA2_3), bvh_taichi.py:179
constexpr int kChunk = 64;          // work items per queue refill (one atomic)

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// a / b is NaN (IEEE): a or b NaN, 0/0 or inf/inf
__device__ __forceinline__ bool div_is_nan(float a, float b) {
    return isnan(a) || isnan(b) || (a == 0.0f && b == 0.0f) || (isinf(a) && isinf(b));
}
// (a.x / b, a.y / b, a.z / b), correctly rounded like IEEE division.  The compiler's
// expansion of one f32 division on gfx950 is
//     v_div_scale (den), v_rcp, 2 fma (reciprocal refinement), v_div_scale (num), mul,
//     3 fma (two quotient corrections, the last as v_div_fmas), v_div_fixup
// and v_div_scale / v_div_fixup change nothing when numerator and denominator are finite
// with |x| in [2^-40, 2^40]: the exponent difference (<= 80) stays below the scaling
// threshold of 96, the denominator, its reciprocal and the quotient are normal, and the
// numerator's biased exponent exceeds 23.  For such operands the remaining sequence
// is therefore bit-identical to the full expansion, and the reciprocal refinement is
// shared by the three quotients of one denominator.  A wave with any lane outside the
// range (zero, tiny, huge, inf, NaN) takes the plain divisions.
// fminf drops a NaN operand, the sum does not: a NaN or inf anywhere fails `sum <= 2^40`
__device__ __forceinline__ bool div3_fast_ok(V3 a, float b) {
    const float lo = fminf(fminf(fabsf(a.x), fabsf(a.y)), fminf(fabsf(a.z), fabsf(b)));
    const float sum = (fabsf(a.x) + fabsf(a.y)) + (fabsf(a.z) + fabsf(b));
    return lo >= 0x1p-40f && sum <= 0x1p40f;
}
__device__ __forceinline__ V3 div3_fast(V3 a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    r = __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
    auto q1 = [&](float n) {
        float q = n * r;
        q = __builtin_fmaf(__builtin_fmaf(-b, q, n), r, q);
        return __builtin_fmaf(__builtin_fmaf(-b, q, n), r, q);
    };
    return v3(q1(a.x), q1(a.y), q1(a.z));
}
__device__ __forceinline__ V3 div3(V3 a, float b) {
    if (__ballot(!div3_fast_ok(a, b)) == 0) return div3_fast(a, b);
    return v3(a.x / b, a.y / b, a.z / b);
}
// (a.x / pdf, a.y / pdf, a.z / pdf) under the reference's NaN rule (tracing.py:146-148): when
// any quotient would be NaN, pdf = 1e-4 instead.  Operands in div3's fast range (finite,
// magnitudes in [2^-40, 2^40]) cannot give a NaN quotient, so a wave whose lanes are all in
// range skips the NaN tests.
__device__ __forceinline__ V3 div3_nan_guard(V3 a, float pdf) {
    if (__ballot(!div3_fast_ok(a, pdf)) == 0) return div3_fast(a, pdf);
    if (div_is_nan(a.x, pdf) || div_is_nan(a.y, pdf) || div_is_nan(a.z, pdf)) pdf = 1e-4f;
    return v3(a.x / pdf, a.y / pdf, a.z / pdf);
}
// v_cmp_class_f32 masks (one VALU instruction tests any set of IEEE classes)
constexpr int kClassNegNormal = 1 << 3, kClassPosZero = 1 << 6, kClassPosNormal = 1 << 8;
constexpr int kClassNormal = kClassNegNormal | kClassPosNormal;
constexpr int kClassDenorm = (1 << 4) | (1 << 7);
// 1 / b, correctly rounded: for finite |b| in [2^-40, 2^40] the division expansion (see
// div3) with numerator 1 is the refined reciprocal plus two quotient corrections
// (its q = 1 * r is exact).
// the sequence itself (prt_selftest_rcp / prt_selftest_guards compare it with the IEEE division
// over all 2^32 floats)
__device__ __forceinline__ float rcp_fast_seq(float b) {
    float r = __builtin_amdgcn_rcpf(b);
    r = __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
    const float q = __builtin_fmaf(__builtin_fmaf(-b, r, 1.0f), r, r);
    return __builtin_fmaf(__builtin_fmaf(-b, q, 1.0f), r, q);
}
// The wave's lanes of class mask m, as one v_cmp_class_f32 into an SGPR pair (inactive lanes read 0).
// Written out because the ballot of llvm.amdgcn.class is lowered through a VGPR (v_cndmask + v_cmp: two
// more VALU per test), and the mask sits in an SGPR (above 64 it is no inline constant; a VGPR copy
// pinned across the loops cost the pooled kernel a spill).
__device__ __forceinline__ uint64_t class_lanes(float x, int m) {
    uint64_t k;
    asm("v_cmp_class_f32_e64 %0, %1, %2" : "=s"(k) : "v"(x), "s"(m));
    return k;
}
// rcp_fast_seq's guard, on the RESULT (round 6): whenever the sequence returns a
// normal float it returns 1.0f / b — proven by the exhaustive sweep over all 2^32 operands on gfx950
// (prt_selftest_guards counter 0 with this per-lane form, tests/test_gpu_selftest.py); zero, denormal,
// huge (> 2^126), infinite and NaN operands give a non-normal result and take the division.  One
// v_cmp_class per test instead of round 5's two range compares on |b|.
__device__ __forceinline__ bool rcp_guard_ok(float r) { return __builtin_amdgcn_classf(r, kClassNormal); }
__device__ __forceinline__ float rcp_exact(float b) {
    float r = rcp_fast_seq(b);
    if (class_lanes(r, kClassNormal) != __builtin_amdgcn_read_exec()) {
        // a real branch: without the (empty, volatile) asm the compiler if-converts the division into
        // every test (both sequences and a select); a non-inlined division here (a cold call) ran 0.2 %
        // slower at C2 (profiles/r06/guards/)
        asm volatile("");
        r = 1.0f / b;
    }
    return r;
}
// Correctly rounded sqrt.  hipcc expands sqrtf on gfx950 as: scale x by 2^32 when
// x < 2^-96, v_sqrt_f32, correct the result by one ulp down / up from the signs of the
// residuals fma(-(s -/+ 1 ulp), s, x), unscale, and return x itself for +-0 / +inf.  With FAST
// a wave whose operands are all in the guard's domain (below) runs the corrected v_sqrt alone
// (bit-identical); other waves take sqrtf.  FAST is used by the LDS-scene kernels (C2 -0.5 %); the
// global-scene kernel keeps sqrtf (its extra live registers cost spills there).
// the sequence itself (prt_selftest_guards sweeps it over all 2^32 floats against sqrtf)
__device__ __forceinline__ float sqrt_fast_seq(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u);
    const float su = __uint_as_float(__float_as_uint(s) + 1u);
    const float rd = __builtin_fmaf(-sd, s, x);
    const float ru = __builtin_fmaf(-su, s, x);
    const float r = rd <= 0.0f ? sd : s;
    return ru > 0.0f ? su : r;
}
// Its guard (round 6): x >= 2^-96, ONE compare instead of round 5's range test
// [2^-96, FLT_MAX].  The exhaustive sweep over all 2^32 floats (prt_selftest_guards counters 4-9)
// finds the sequence equal to sqrtf for every operand except the denormals (of either sign) and the
// operands in [+0, 2^-96), where sqrtf scales: +inf gives +inf on both sides, negative operands and NaN
// give NaN on both sides, so the upper bound was never needed.
__device__ __forceinline__ bool sqrt_guard_ok(float x) { return x >= 0x1p-96f; }
template <bool FAST>
__device__ __forceinline__ float sqrt_cr(float x) {
    if constexpr (FAST) {
        if (__ballot(!sqrt_guard_ok(x)) == 0) return sqrt_fast_seq(x);
        asm volatile("");
    }
    return sqrtf(x);
}
// taichi_glsl normalize: v / length(v) (IEEE division, correctly rounded sqrt).
// FAST (round 6): the shared-reciprocal quotients under a cheaper guard than div3's — every |a_i| >=
// 2^-60 and s = length(a) <= 2^64 (four compares, no min / sum chain).  That is
// div3's no-scaling condition for this quotient: s >= |a_i| (1 - 2^-23) > 2^-61 (s = sqrt(dot) and
// dot >= each rounded square), so s and 1/s are normal, |a_i / s| <= 1 + 2^-23 (no overflow, exponent
// difference <= 1 < 96), |a_i / s| >= 2^-124 (normal with two binades of margin), every a_i has a
// biased exponent >= 67 > 23 and none is zero; an infinite a_i makes s infinite and a NaN fails its
// compare, so those waves divide.
template <bool FAST = false>
__device__ __forceinline__ V3 normalize(V3 a) {
    const float s = sqrt_cr<FAST>(dot(a, a));
    if constexpr (FAST) {
        const bool ok = (int)(fabsf(a.x) >= 0x1p-60f) & (int)(fabsf(a.y) >= 0x1p-60f) &
                        (int)(fabsf(a.z) >= 0x1p-60f) & (int)(s <= 0x1p64f);
        if (__ballot(!ok) == 0) return div3_fast(a, s);
        return v3(a.x / s, a.y / s, a.z / s);
    }
    return div3(a, s);
}
__device__ __forceinline__ V3 xyz(float4 f) { return v3(f.x, f.y, f.z); }
// The Lambert vertex's BRDF weight division (att * max(cw, 0)) / (|cw| / pi) under the reference's NaN
// rule (tracing.py:146-148; ad = att * dz, pdf = |cw| * InvPi).  FAST (round 6):
// on a scene whose albedos lie in [2^-40, 2^40] and whose face normals have length in [0.5, 2]
// (TraceParams::shade_fast, checked on the host), cw >= 2^-60 alone puts the quotient in div3's
// no-scaling domain.  Numerator and denominator both carry cw, so the quotient ad_i / pdf ~ pi att_i lies
// in [2^-39, 2^42] (normal, exponent difference <= 42 < 96) whatever cw is; cw only has to keep the
// operands themselves in range: pdf = cw / pi >= 2^-62 and ad_i = att_i cw >= 2^-100 are normal (biased
// exponent >= 27 > 23, non-zero), and for cw < 2^87 ad_i < 2^127 is finite and 1 / pdf normal.  No
// quotient is NaN, so the rule does not fire: one compare instead of div3's range test (a NaN cw fails
// it).  A triangle's cw <= |n| |wi| <= 2 (wi normalised).  A sphere's normal (p - c) / r is NOT near unit
// length and the host checks nothing about it: p = o + d t is rounded at the size of |o| + |d| t and the
// root's discriminant cancels, so |p - c| reaches about 2^-11 of the ray's length whatever r is.
// tests/test_hard_spheres.py records lengths of 0.0064 .. 108 (r = 1e-3 hit from 200 away), 0.49 .. 8658
// (r = 1e-4 from 2000) and 0.019 .. 9.9 (r = 1e-4 from 2), outside [0.5, 2] on 2200, 1558 and 2072 of
// some 3000 hits each; the bound cw < 2^87 leaves 73 binades above the largest of them, and
// tests/test_gpu_hard_spheres.py holds every such path to the oracle's bits in every kernel variant.  (A
// cw of 2^87 takes a sphere of r < 2^-98 of its hit distance: an infinite cw passes the compare, and
// there the sequence gives NaN where the rule gives inf.)
template <bool FAST>
__device__ __forceinline__ V3 lambert_div(V3 ad, float pdf, float cw, int shade_fast) {
    if constexpr (FAST) {
        if (shade_fast && __ballot(!(cw >= 0x1p-60f)) == 0) return div3_fast(ad, pdf);
    }
    return div3_nan_guard(ad, pdf);
}
// The NEE term's division (em * dot1 * dot2) / |p - p2|^2 (tracing.py:92-108).  FAST (round 6): under
// shade_fast (above) em_i in [2^-40, 2^40] and dot2 <= 2 (unit-ish w, the light triangle's normal of length
// <= 2), and dot1 <= |n| with |n| <= 2 at a triangle, so with dot1, dot2 >= 2^-20 and sl in [2^-40, 2^40]
// the numerators lie in [2^-81, 2^42] (normal, biased exponent >= 46), sl and 1 / sl are normal, the
// quotients lie in [2^-121, 2^82] and the exponent difference is <= 82 < 96: div3's no-scaling domain
// with four compares instead of div3's range test.  At a sphere dot1 <= |n| has no such bound (see
// lambert_div); every factor of |n| adds to the numerator alone, so the same argument holds for |n| <=
// 2^13 (numerators below 2^55, quotients below 2^95, exponent difference <= 95) and, with the rows and
// distances a scene really has, far beyond: the largest numerator is max(em_i) dot1 dot2, and the
// margin is 96 - log2 of that over sl.  The longest normal tests/test_hard_spheres.py records is 8658 =
// 2^13.1, on rows of em = 1 at sl > 2^-7 (exponent difference <= 22); tests/test_gpu_hard_spheres.py
// holds those paths to the oracle's bits.  Beyond the margin the sequence still divides correctly
// unless an intermediate of it leaves the normal range, which is what v_div_scale exists for.
template <bool FAST>
__device__ __forceinline__ V3 nee_div(V3 a, float sl, float dot1, float dot2, int shade_fast) {
    if constexpr (FAST) {
        const bool ok = (int)(dot1 >= 0x1p-20f) & (int)(dot2 >= 0x1p-20f) & (int)(sl >= 0x1p-40f) &
                        (int)(sl <= 0x1p40f);
        if (shade_fast && __ballot(!ok) == 0) return div3_fast(a, sl);
    }
    return div3(a, sl);
}


// ------------------------------------------------------------------ RNG spec
__device__ __forceinline__ uint32_t pcg_permute(uint32_t s) {
    uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ uint32_t pcg_hash(uint32_t v) { return pcg_permute(v * 747796405u + 2891336453u); }
__device__ __forceinline__ uint32_t rng_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel, uint32_t sample) {
    uint32_t h = pcg_hash(seed_lo);
    h = pcg_hash(h ^ seed_hi ^ pixel);
    return pcg_hash(h + sample);
}
__device__ __forceinline__ float rng_next(uint32_t& st) {
    st = st * 747796405u + 2891336453u;
    return (float)(pcg_permute(st) >> 8) * 0x1p-24f;
}
// taichi_glsl randInt(a, b), inclusive
__device__ __forceinline__ int rng_int(uint32_t& st, int a, int b) {
    float u = rng_next(st);
    int k = (int)floorf(u * (float)(b - a + 1));
    k = k > b - a ? b - a : k;
    return a + k;
}

// --------------------------------------------- concentric disk (samplers.py:9-32)
__device__ __forceinline__ float poly_sin(float x) {
    float z = x * x;
    return ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * x + x;
}
__device__ __forceinline__ float poly_cos(float x) {
    float z = x * x;
    return ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z
           - 0.5f * z + 1.0f;
}
template <bool FAST = false>
__device__ __forceinline__ V3 cosine_hemisphere(float u0, float u1) {
    float ox = 2.0f * u0 - 1.0f, oy = 2.0f * u1 - 1.0f;
    float dx = 0.0f, dy = 0.0f;
    if (!(ox == 0.0f && oy == 0.0f)) {
        // |ox| > |oy|: r = ox, theta = pi/4 (oy/ox), (c, s) = (cos, sin)(theta);
        // else:        r = oy, a = pi/4 (ox/oy), theta = pi/2 - a, (c, s) = (sin, cos)(a).
        // Both cases as one division and one polynomial pair on selected operands (a
        // divergent if/else would run two of each on a wave holding both cases).
        const bool wide = fabsf(ox) > fabsf(oy);
        const float r = wide ? ox : oy;
        float t;
        if constexpr (FAST) {
            // round 6: the quotient by div3's shared-reciprocal sequence, unguarded: u0, u1 are
            // rng_next draws (multiples of 2^-24 in [0, 1)), so ox, oy = 2u - 1 are exact multiples of
            // 2^-23 in [-1, 1): |r| >= 2^-23 and the numerator is +0 or of magnitude in [2^-23, |r|] —
            // div3's no-scaling domain (quotient in [2^-23, 1], biased exponents >= 104), and for
            // the numerator +0 the sequence returns the IEEE zero of sign(r) itself
            const float q = wide ? oy : ox;
            float rr = __builtin_amdgcn_rcpf(r);
            rr = __builtin_fmaf(__builtin_fmaf(-r, rr, 1.0f), rr, rr);
            float qq = q * rr;
            qq = __builtin_fmaf(__builtin_fmaf(-r, qq, q), rr, qq);
            t = kPiOver4 * __builtin_fmaf(__builtin_fmaf(-r, qq, q), rr, qq);
        } else {
            t = kPiOver4 * ((wide ? oy : ox) / r);
        }
        const float pc = poly_cos(t), ps = poly_sin(t);
        dx = r * (wide ? pc : ps);
        dy = r * (wide ? ps : pc);
    }
    float m = 1.0f - dx * dx - dy * dy;
    return v3(dx, dy, sqrt_cr<FAST>(m > 0.0f ? m : 0.0f));
}

// rotate_z_to + rotate_vector (mat4_taichi.py:9-60): rows (x, z, n)
__device__ __forceinline__ V3 to_world(V3 n, V3 l) {
    V3 v = normalize(n);
    V3 r1, r2, r3;
    if (v.y == 1.0f) {
        r1 = v3(1, 0, 0); r2 = v3(0, 0, 1); r3 = v3(0, 1, 0);
    } else if (v.y == -1.0f) {
        r1 = v3(1, 0, 0); r2 = v3(0, 0, 1); r3 = v3(0, -1, 0);
    } else {
        V3 x = normalize(cross(v, v3(0.0f, 1.0f, 0.0f)));
        V3 z = normalize(cross(x, v));
        r1 = x; r2 = z; r3 = v;
    }
    return normalize(r1 * l.x + r2 * l.y + r3 * l.z);
}

// ------------------------------------------------------- camera (camera_taichi.py:47-74)
__device__ __forceinline__ void gen_ray(const float* cam, float u, float v, uint32_t& st, V3& o, V3& d) {
    const float sd0 = cam[16], sd1 = cam[17], sd2 = cam[18], sd3 = cam[19];
    float rd[4] = {(u - 0.5f) * sd0 / 0.5f, (v - 0.5f) * sd1 / 0.5f, -sd2, 1.0f};
    float ro[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    if (sd3 > 0.0f) {
        ro[0] = sd2 * rng_next(st) - sd2 / 2.0f;
        ro[1] = sd2 * rng_next(st) - sd2 / 2.0f;
    }
    float dw[4], ow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* c = cam + 4 * i;
        dw[i] = rd[0] * c[0] + rd[1] * c[1] + rd[2] * c[2] + rd[3] * c[3];
        ow[i] = ro[0] * c[0] + ro[1] * c[1] + ro[2] * c[2] + ro[3] * c[3];
    }
    float f0 = dw[0] - ow[0], f1 = dw[1] - ow[1], f2 = dw[2] - ow[2], f3 = dw[3] - ow[3];
    float l = sqrtf(f0 * f0 + f1 * f1 + f2 * f2 + f3 * f3);
    o = v3(ow[0], ow[1], ow[2]);
    d = v3(f0 / l, f1 / l, f2 / l);
}

// -------------------------------------- specular helpers (bsdf_taichi.py:6-22)
__device__ __forceinline__ float schlick(float cosine, float idx) {
    float r0 = (1.0f - idx) / (1.0f + idx);
    r0 = r0 * r0;
    float m = 1.0f - cosine;
    return r0 + (1.0f - r0) * (m * m * m * m * m);
}
__device__ __forceinline__ V3 reflect3(V3 v, V3 n) { return v - n * (2.0f * dot(v, n)); }
__device__ __forceinline__ V3 refract3(V3 v, V3 n, float eta) {
    float ct = -dot(v, n);
    ct = ct > 1.0f ? 1.0f : ct;
    V3 perp = (v + n * ct) * eta;
    float k = 1.0f - dot(perp, perp);
    return perp + n * (-sqrtf(fabsf(k)));
}
// random_in_unit_sphere (vec3_taichi.py:299-306) with deterministic ops: see oracle
__device__ __forceinline__ float cbrt_spec(float x) {
    if (!(x > 0.0f)) return 0.0f;
    float y = __uint_as_float(__float_as_uint(x) / 3u + 709921077u);
    for (int i = 0; i < 3; ++i) y = (2.0f * y + x / (y * y)) / 3.0f;
    return y;
}
__device__ __forceinline__ V3 random_in_unit_sphere(uint32_t& st) {
    float u1 = rng_next(st), u2 = rng_next(st), u3 = rng_next(st);
    int q = (int)floorf(u1 * 4.0f + 0.5f);
    float a = 6.28318530717958647692f * (u1 - 0.25f * (float)q);
    float pc = poly_cos(a), ps = poly_sin(a);
    float c, sn;
    switch (q & 3) {
        case 0: c = pc; sn = ps; break;
        case 1: c = -ps; sn = pc; break;
        case 2: c = -pc; sn = -ps; break;
        default: c = ps; sn = -pc; break;
    }
    float z = 2.0f * u2 - 1.0f;
    float m = 1.0f - z * z;
    float sp = sqrtf(m > 0.0f ? m : 0.0f);
    float r = cbrt_spec(u3);
    return v3(r * sp * c, r * sp * sn, r * z);
}
// hit_sphere (intersection_taichi.py:15-36): nearest root in [t_min, t_max], else far root
__device__ __forceinline__ bool sphere_hit(float4 sc, V3 o, V3 d, float t_min, float t_max, float& root) {
    V3 oc = o - xyz(sc);
    float a = dot(d, d);
    float half_b = dot(oc, d);
    float cc = dot(oc, oc) - sc.w * sc.w;
    float disc = half_b * half_b - a * cc;
    if (!(disc >= 0.0f)) return false;
    float sq = sqrtf(disc);
    root = (-half_b - sq) / a;
    if (root < t_min || t_max < root) {
        root = (-half_b + sq) / a;
        if (root < t_min || t_max < root) return false;
    }
    return true;
}

}  // namespace
}  // namespace prt

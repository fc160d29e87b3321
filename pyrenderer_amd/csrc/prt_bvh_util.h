// prt_bvh_util.h — the small pieces the two builder units share (prt_bvh.cpp: the BVH2; prt_bvh4.cpp:
// the collapse and the quantiser) with the device refit (prt_refit.hip), which must reproduce the host's
// words: the rounding helpers and the quantiser of one four-wide node compile on both sides.  Standard
// library only.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIP__)
#define PRT_UTIL_HD __attribute__((host)) __attribute__((device))
#else
#define PRT_UTIL_HD
#endif

namespace prt {

constexpr int32_t kEmptyRef = 0x7FFFFFFF;   // ref of an empty slot of a wide node: the traversal sentinel

// surface area of the box (lo, hi), f32 or f64 corners, in double
template <class T>
inline double box_area(const T* lo, const T* hi) {
    double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// the f32 at or below / at or above x
PRT_UTIL_HD inline float round_down_f32(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -INFINITY);
    return f;
}
PRT_UTIL_HD inline float round_up_f32(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}

// the bits of one 4-byte type as another (node records keep child references in float lanes)
template <class To, class From>
PRT_UTIL_HD inline To bits(From v) {
    static_assert(sizeof(To) == sizeof(From), "bits: same size");
    To t;
    std::memcpy(&t, &v, sizeof t);
    return t;
}

// The quantised record q (16 floats, prt_internal.h kNodeQF4) of the four-wide node f (32 floats): per axis
// the origin rounded down to f32 and the grid step = the f32 at or above range / 254 (and >= 1e-30), the
// child planes floored / ceiled on that grid with the margin 2 pad.  All in f64 but for the two roundings;
// no multiply-add to contract.  quantize_bvh4 on the host and the refit on the device both call it.
PRT_UTIL_HD inline void quantize_node4(const float* f, float pad, float* q) {
    const double margin = 2.0 * (double)pad;
    bool ok[4];
    for (int k = 0; k < 4; ++k) ok[k] = std::isfinite(f[k]);   // empty slots hold +inf
    for (int a = 0; a < 3; ++a) {
        uint32_t ql = 0, qh = 0;
        double lo = INFINITY, hi = -INFINITY;
        for (int k = 0; k < 4; ++k)
            if (ok[k]) {
                const double l = (double)f[(2 * a) * 4 + k], h = (double)f[(2 * a + 1) * 4 + k];
                lo = l < lo ? l : lo;
                hi = hi < h ? h : hi;
            }
        if (!(lo <= hi)) { lo = 0.0; hi = 0.0; }
        const float o = round_down_f32(lo - margin);
        const double ext = hi + margin - (double)o;
        const float up = round_up_f32(ext / 254.0);
        const float stf = up < (float)1e-30 ? (float)1e-30 : up;
        const double st = (double)stf;
        q[a] = o;
        q[3 + a] = stf;
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            const double l = (double)f[(2 * a) * 4 + k], h = (double)f[(2 * a + 1) * 4 + k];
            long long ql_k = (long long)std::floor((l - margin - (double)o) / st);
            long long qh_k = (long long)std::ceil((h + margin - (double)o) / st);
            ql_k = ql_k < 0 ? 0 : ql_k > 255 ? 255 : ql_k;
            qh_k = qh_k < 0 ? 0 : qh_k > 255 ? 255 : qh_k;
            ql |= (uint32_t)ql_k << (8 * k);
            qh |= (uint32_t)qh_k << (8 * k);
        }
        q[6 + 2 * a] = bits<float>(ql);
        q[7 + 2 * a] = bits<float>(qh);
    }
    for (int k = 0; k < 4; ++k) q[12 + k] = ok[k] ? f[24 + k] : bits<float>(kEmptyRef);
}

}  // namespace prt

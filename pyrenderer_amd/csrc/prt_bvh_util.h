// prt_bvh_util.h — the small pieces the two builder units share (prt_bvh.cpp: the BVH2; prt_bvh4.cpp:
// the collapse and the quantiser).  Standard library only.
#pragma once
#include <cmath>
#include <cstring>

namespace prt {

// surface area of the box (lo, hi), f32 or f64 corners, in double
template <class T>
inline double box_area(const T* lo, const T* hi) {
    double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// the f32 at or below / at or above x
inline float round_down_f32(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -INFINITY);
    return f;
}
inline float round_up_f32(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}

// the bits of one 4-byte type as another (node records keep child references in float lanes)
template <class To, class From>
inline To bits(From v) {
    static_assert(sizeof(To) == sizeof(From), "bits: same size");
    To t;
    std::memcpy(&t, &v, sizeof t);
    return t;
}

}  // namespace prt

// prt_refit.hip — refit of a resident scene's trees on the device after its primitives moved
// (prt_scene_update, prt_scene.cpp).  Topology, leaf references and triangle order stay those
// of creation; three kernel groups rewrite what a motion changes: the BVH-order triangle records with each
// slot's bounds, the child boxes of the four- and eight-wide trees bottom-up, one launch per tree level (a
// kernel boundary orders a level after the one below it: the XCDs' L2s are not coherent within a launch),
// and the quantised four-wide records.  Every word equals what the host builder writes for the same tree
// and geometry (flatten in prt_bvh.cpp, emit_wide and quantize_bvh4 in prt_bvh4.cpp), so the unit is built
// with the library's -ffp-contract=off and shares quantize_node4 with the host (prt_bvh_util.h).
#include "prt_refit.h"

#include "prt_bvh_util.h"
#include "prt_internal.h"

namespace prt {
namespace {

constexpr int kRefitBlock = 256;

inline unsigned refit_grid(int64_t n) { return (unsigned)((n + kRefitBlock - 1) / kRefitBlock); }

__global__ void __launch_bounds__(kRefitBlock)
refit_tris_kernel(const float* __restrict__ tri_v, const int32_t* __restrict__ order, int64_t n_slots,
                  float4* __restrict__ tris, float* __restrict__ bounds) {
    const int64_t s = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (s >= n_slots) return;
    const int32_t t = order[s];
    const float* v = tri_v + 9 * (int64_t)t;
    float p[9];
    for (int k = 0; k < 9; ++k) p[k] = v[k];
    // e1 = v1 - v0, e2 = v2 - v0 in f32, the id in the first record's w: flatten()'s words
    tris[3 * s] = make_float4(p[0], p[1], p[2], bits<float>(t));
    tris[3 * s + 1] = make_float4(p[3] - p[0], p[4] - p[1], p[5] - p[2], 0.0f);
    tris[3 * s + 2] = make_float4(p[6] - p[0], p[7] - p[1], p[8] - p[2], 0.0f);
    // the bounds of the vertices themselves, not of v0 + e: the builder boxes the vertices
    float* b = bounds + 6 * s;
    for (int k = 0; k < 3; ++k) {
        const float lo01 = p[3 + k] < p[k] ? p[3 + k] : p[k], hi01 = p[k] < p[3 + k] ? p[3 + k] : p[k];
        b[k] = p[6 + k] < lo01 ? p[6 + k] : lo01;
        b[3 + k] = hi01 < p[6 + k] ? p[6 + k] : hi01;
    }
}

// Plane p (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) of child k at float (k / 4) * 24 + 4 p + k % 4, the refs after
// the last group (emit_wide).  A node only reads nodes of the level below and the slot bounds, and only
// writes its own boxes: no two threads of a launch touch the same word.  Refs are never written.
template <int kWidth>
__global__ void __launch_bounds__(kRefitBlock)
refit_level_kernel(float* __restrict__ nodes, const int32_t* __restrict__ level, int64_t n,
                   const float* __restrict__ bounds, float pad) {
    constexpr int kNode = kWidth == 4 ? kNode4F4 * 4 : kNode8F4 * 4;
    const int64_t i = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    float* f = nodes + (size_t)level[i] * kNode;
    for (int k = 0; k < kWidth; ++k) {
        const int32_t ref = bits<int32_t>(f[6 * kWidth + k]);
        if (ref == kEmptyRef) continue;   // keeps its inverted box
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (ref < 0) {
            const int64_t first = leaf_first(ref);
            const int count = leaf_count(ref);
            for (int j = 0; j < count; ++j) {
                const float* b = bounds + 6 * (first + j);
                for (int a = 0; a < 3; ++a) {
                    lo[a] = b[a] < lo[a] ? b[a] : lo[a];
                    hi[a] = hi[a] < b[3 + a] ? b[3 + a] : hi[a];
                }
            }
            for (int a = 0; a < 3; ++a) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
        } else {
            const float* c = nodes + (size_t)ref * kNode;
            for (int j = 0; j < kWidth; ++j) {
                if (bits<int32_t>(c[6 * kWidth + j]) == kEmptyRef) continue;
                const int at = (j / 4) * 24 + j % 4;
                for (int a = 0; a < 3; ++a) {
                    const float l = c[at + (2 * a) * 4], h = c[at + (2 * a + 1) * 4];
                    lo[a] = l < lo[a] ? l : lo[a];
                    hi[a] = hi[a] < h ? h : hi[a];
                }
            }
        }
        const int at = (k / 4) * 24 + k % 4;
        for (int a = 0; a < 3; ++a) {
            f[at + (2 * a) * 4] = lo[a];
            f[at + (2 * a + 1) * 4] = hi[a];
        }
    }
}

__global__ void __launch_bounds__(kRefitBlock)
refit_quantize_kernel(const float* __restrict__ nodes4, int64_t n, float pad, float* __restrict__ nodes4q) {
    const int64_t i = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    float f[kNode4F4 * 4], q[kNodeQF4 * 4];
    for (int k = 0; k < kNode4F4 * 4; ++k) f[k] = nodes4[(size_t)i * (kNode4F4 * 4) + k];
    quantize_node4(f, pad, q);
    for (int k = 0; k < kNodeQF4 * 4; ++k) nodes4q[(size_t)i * (kNodeQF4 * 4) + k] = q[k];
}

}  // namespace

hipError_t launch_refit_tris(const float* tri_v, const int32_t* order, int64_t n_slots, float4* tris, float* bounds,
                             hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_tris_kernel, dim3(refit_grid(n_slots)), dim3(kRefitBlock), 0, stream, tri_v, order, n_slots,
                       tris, bounds);
    return hipGetLastError();
}

hipError_t launch_refit_level(int width, float* nodes, const int32_t* level, int64_t n, const float* bounds, float pad,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (width == 8)
        hipLaunchKernelGGL(refit_level_kernel<8>, dim3(refit_grid(n)), dim3(kRefitBlock), 0, stream, nodes, level, n,
                           bounds, pad);
    else
        hipLaunchKernelGGL(refit_level_kernel<4>, dim3(refit_grid(n)), dim3(kRefitBlock), 0, stream, nodes, level, n,
                           bounds, pad);
    return hipGetLastError();
}

hipError_t launch_refit_quantize(const float* nodes4, int64_t n, float pad, float* nodes4q, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(refit_quantize_kernel, dim3(refit_grid(n)), dim3(kRefitBlock), 0, stream, nodes4, n, pad, nodes4q);
    return hipGetLastError();
}

}  // namespace prt

// prt_refit.h — launch interface of the device refit of a resident scene (prt_refit.hip; prt_scene_update in
// prt_scene.cpp enqueues it).  Internal to libprt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prt {

// Triangle records of the n_slots BVH slots from the original-order vertices tri_v (n_tri x 9): slot s holds
// triangle order[s] as (v0, id bits) (v1 - v0, 0) (v2 - v0, 0), and bounds[6 s ..] = min xyz, max xyz of its
// three vertices.
hipError_t launch_refit_tris(const float* tri_v, const int32_t* order, int64_t n_slots, float4* tris, float* bounds,
                             hipStream_t stream);
// One level of the wide tree of `width` (4 or 8) children per node: the child boxes of the n nodes level[0..n)
// from the slot bounds (leaf children, padded) and from the child nodes' boxes (inner children).  The caller
// enqueues the levels deepest first on one stream: the kernel boundary orders a level after the one below it.
hipError_t launch_refit_level(int width, float* nodes, const int32_t* level, int64_t n, const float* bounds, float pad,
                              hipStream_t stream);
// quantised records (prt_internal.h kNodeQF4) of the n four-wide nodes: quantize_node4 per node
hipError_t launch_refit_quantize(const float* nodes4, int64_t n, float pad, float* nodes4q, hipStream_t stream);

}  // namespace prt

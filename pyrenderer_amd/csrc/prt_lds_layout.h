// prt_lds_layout.h — the LDS layout of each trace kernel, stated once: the kernels take their region
// pointers from it and the host takes the launch's dynamic LDS size from it (prt_plan.h
// trace_smem_bytes), which also decides lds_fits and the default variant.  Standard library only, no HIP
// include: prt_plan.cpp and tools/sanitize/host_check.cpp compile it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIP__)
#define PRT_HD __host__ __device__
#else
#define PRT_HD
#endif

namespace prt {

constexpr int kBlock = 256;                    // threads of a trace block: every layout below is per block
constexpr int kPoolF4 = 7 * kBlock / 4;        // pool SoA: 7 x 256 f32
constexpr int kQueueF4 = 2 * kBlock / 16;      // queue: 2 x 256 u8, by iteration parity
constexpr int kCtlF4 = 3;                      // ctl: 12 words

// The sizes the layouts depend on.  width: children per node of the tree the kernel traverses in LDS (4:
// the BVH4; 8: the BVH8 of prt_internal.h).  n_node_f4 counts the float4 of that tree's global nodes — 8
// per BVH4 node, 14 per BVH8 node — and is a multiple of that (the collapse writes whole nodes): the LDS
// copy holds 8 octant copies of 7 (14) float4 per node, 56 * (n_node_f4 / 8) or 112 * (n_node_f4 / 14)
// float4, which node_copy_f4 writes as 7 * n_node_f4 or 8 * n_node_f4 — equal under that precondition only.
// n_tri_f4: 3 float4 per triangle record in BVH order; n_mat: materials of 8 floats; n_lt: emitter
// triangles of 4 float4; n_light: lights (n_light + 1 prefix offsets); stack: traversal stack entries per
// lane.
struct LdsSizes { int n_node_f4, n_tri_f4, n_tri, n_mat, n_lt, n_light, stack, width = 4; };
PRT_HD constexpr int64_t node_copy_f4(const LdsSizes& z) { return (z.width == 8 ? 8 : 7) * (int64_t)z.n_node_f4; }
// nodes of the tree (lds_fits: node indices fit the 16-bit stack entries)
PRT_HD constexpr int64_t node_count(const LdsSizes& z) { return z.n_node_f4 / (z.width == 8 ? 14 : 8); }

// float4 of a block's traversal stacks with 16-bit entries (LDS-resident scenes) ...
PRT_HD constexpr int64_t stack16_f4(int stack) { return (int64_t)stack * kBlock * 2 / 16; }
// ... and bytes of those with 32-bit entries, all the LDS of the global-scene trace kernel (the LDS part
// of its spill stack) and of the hit-query kernels
PRT_HD constexpr size_t stack32_bytes(int stack) { return (size_t)stack * kBlock * 4; }

// trace_kernel with the scene in LDS: float4 offsets of its regions in order, and the total in bytes.
// The light offsets are n_light + 1 words at the very end (no padding to a float4).
struct TraceLds {
    int64_t stacks, nodes, tris, normals, frames, mats, light_v, light_off;
    size_t bytes;
};
PRT_HD constexpr TraceLds trace_lds(const LdsSizes& z) {
    TraceLds l{};
    l.stacks = 0;
    l.nodes = l.stacks + stack16_f4(z.stack);
    l.tris = l.nodes + node_copy_f4(z);
    l.normals = l.tris + z.n_tri_f4;                 // one float4 per triangle
    l.frames = l.normals + z.n_tri;                  // 2 x 3 float4 per triangle
    l.mats = l.frames + 6 * (int64_t)z.n_tri;
    l.light_v = l.mats + 2 * (int64_t)z.n_mat;
    l.light_off = l.light_v + 4 * (int64_t)z.n_lt;
    l.bytes = 16 * (size_t)l.light_off + 4 * ((size_t)z.n_light + 1);
    return l;
}

// trace_kernel_pool: stacks of z.stack 16-bit entries, the shadow pool, queue and control words, then
// the scene copy without normals and frames; the light offsets are padded to whole float4 ahead of the
// materials.
struct PoolLds {
    int64_t stacks, pool, queue, ctl, nodes, tris, light_v, light_off, mats;
    size_t bytes;
};
PRT_HD constexpr PoolLds pool_lds(const LdsSizes& z) {
    PoolLds l{};
    l.stacks = 0;
    l.pool = l.stacks + stack16_f4(z.stack);
    l.queue = l.pool + kPoolF4;
    l.ctl = l.queue + kQueueF4;
    l.nodes = l.ctl + kCtlF4;
    l.tris = l.nodes + node_copy_f4(z);
    l.light_v = l.tris + z.n_tri_f4;
    l.light_off = l.light_v + 4 * (int64_t)z.n_lt;
    l.mats = l.light_off + ((int64_t)z.n_light + 4) / 4;
    l.bytes = 16 * (size_t)(l.mats + 2 * (int64_t)z.n_mat);
    return l;
}

}  // namespace prt

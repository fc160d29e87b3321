// prt_plan.h — the host arithmetic of libprt that needs no GPU: scene argument checks and packing,
// environment knobs, tile and window arithmetic, the launch-chunk plan and the camera's host-evaluated
// terms, and the launch decisions that depend on a scene's sizes alone (LDS footprints, the variant
// choice).  Standard library + prt_internal.h, prt_lds_layout.h and prt_variant_table.h only (no HIP
// include), plain arrays and small structs in and out, so tools/sanitize/host_check.cpp runs all of it
// on the CPU under ASan + UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "prt_internal.h"
#include "prt_lds_layout.h"
#include "prt_variant_table.h"

namespace prt {

// the scene arrays as prt_scene_create receives them (include/prt.h)
struct SceneArgs {
    const float* tri_v; const float* tri_n; const int32_t* tri_mat; int64_t n_tri;
    const float* sph; const int32_t* sph_mat; int64_t n_sph;
    const float* mat; int32_t n_mat;
    const int32_t* light_tri; const int32_t* light_off; int32_t n_light;
};
// prt_scene_create's argument checks, in its order; false: *err holds the message of the first one failed
bool validate_scene(const SceneArgs& a, std::string* err);

struct PackedScene {
    std::vector<float> tri_nm;     // per triangle: (face normal xyz, material id bits)
    std::vector<float> tri_frame;  // per triangle: rotate_z_to rows (x, z, v) of n and of -n, 2 x 12 floats
    std::vector<float> light_v;    // per emitter triangle: V0, V1, V2, (normal xyz, material id bits)
    int n_lt = 0;                  // emitter triangles
    bool plain = false;            // no spheres, no metal / dielectric material (TraceParams::plain)
    bool shade_fast = false;       // TraceParams::shade_fast
};
void pack_scene(const SceneArgs& a, PackedScene* out);   // of validated arguments

// prt_scene_update's argument checks on the new geometry (the counts are those of creation): NULL arrays, a
// vertex or normal that is not finite, a sphere row that is not finite or whose radius is not > 0
bool validate_update(const float* tri_v, const float* tri_n, int64_t n_tri, const float* sph, int64_t n_sph,
                     std::string* err);
// The nodes of a wide tree (prt_internal.h Bvh4Host / Bvh8Host records, `width` 4 or 8) by level, the root
// at level 0: list = the node indices level by level, those of level l at off[l] .. off[l + 1].  emit_wide
// numbers every child above its parent, so one forward sweep finds every depth.  false (never for a tree of
// the library's own): a child reference that is out of range or not above its parent.
bool wide_levels(const float* nodes, int64_t n_nodes, int width, std::vector<int32_t>* list,
                 std::vector<int64_t>* off);

// ---- the host bookkeeping of a device build (prt_scene_rebuild; prt_lbvh.h)
// slots a device build accepts: leaf_ref addresses first < 2^28
constexpr int64_t kLbvhMaxSlots = (int64_t)1 << 28;
// Nodes a wide tree over n slots can have at the most, the room its item and node arrays get before the tree
// is known: every node but a leaf-only root covers a distinct range of two slots or more, and such ranges,
// nested or disjoint, number at most n - 1.
inline int64_t lbvh_node_capacity(int64_t n) { return n > 1 ? n - 1 : 1; }
// bytes of the build's work arrays at n slots (prt_host.h RebuildState), 16 at the least each
struct LbvhScratch { size_t cen, word, key, item, count; };
LbvhScratch lbvh_scratch(int64_t n);
// A tree numbered breadth-first as it is emitted: off[l] .. off[l + 1] are the nodes of level l.
struct LbvhLevels {
    std::vector<int64_t> off{0};
    int64_t n_nodes() const { return off.back(); }
    int depth() const { return (int)off.size() - 2; }          // levels - 1; -1 before the root's level
    // the next level holds `count` nodes (the inner children of the level before, one for the root); false: the
    // count is negative or above `widest`, or the tree would outgrow `capacity` nodes
    bool push(int64_t count, int64_t capacity, int64_t widest);
};
// emit_wide's rule: the sentinel, the ancestors' entries of the deepest node, and the width - 1 slots a visit
// writes above the top
inline int wide_stack_need(int max_anc, int width) { return 1 + max_anc + (width - 1); }
// the level list of such a tree: 0, 1, ..., n_nodes - 1
std::vector<int32_t> iota_list(int64_t n_nodes);

// integer environment knob: `fallback` when unset, else its value clamped to [lo, hi]
long long env_int(const char* name, long long lo, long long hi, long long fallback);
// PRT_SPILL_LDS takes 4, 16 or 32 entries; every other value means 16
inline int spill_lds_entries(long long v) { return v == 4 ? 4 : v == 32 ? 32 : 16; }

// per-tile pixel origins (x0 << 16 | y0) of tile ids in a frame of tiles_x columns of tw x th tiles; a
// padding slot (id -1) gets x0 = 0xFFFF, past any frame's width (<= 65535), so the scatter drops its pixels
std::vector<uint32_t> tile_origins(const int32_t* ids, int64_t n, int tiles_x, int tw, int th);
// tile ids of a window, ascending (tiles of tw x th in the W-wide frame)
std::vector<int32_t> window_tiles(int W, int x0, int y0, int w, int h, int tw, int th);
// 'latin' tile owner of device_scene.tile_owner: rank = (tx + s * ty) mod n with s the
// integer nearest 0.38 n that is coprime with n (every rank owns tiles in every row)
int latin_stride(int n);
std::vector<std::vector<int32_t>> latin_tile_ids(int W, int H, int tile, int n_ranks);   // per rank, ascending
// slot -> pixel as the kernels map it (pixel_of): tile-major, then row-major within the tile
bool slot_in_frame(const std::vector<uint32_t>& origins, int64_t slot, int tw, int th, int W, int H);

// Launches of a render of T samples (spp * n_frames) of n_slots pixels at bytes_per_sample each: as many
// samples per launch as the budget holds (at least one), every launch's item count below 2^31 (32-bit
// work counter), then equal launches: no short last launch paying a whole launch tail for a few samples.
struct ChunkPlan { int64_t chunk, n_launches; };
ChunkPlan plan_chunks(int64_t T, int64_t n_slots, int64_t bytes_per_sample, size_t budget);
// the frames [f0, f1) that the launch samples [s0, s0 + n) overlap (frame f = samples [f spp, (f + 1) spp))
struct FrameSpan { int64_t f0, f1; };
FrameSpan launch_frames(int64_t s0, int64_t n, int64_t spp, int64_t n_frames);

// ---- launch decisions that follow from the scene's sizes alone (prt_lds_layout.h, prt_variant_table.h)
// look-ups in the variant table; unknown ids answer false
bool variant_pool(int var);
bool variant_mis(int var);
bool variant_uses_lds(int var);
bool variant_spills(int var);      // the global-scene trace kernels traverse quantised nodes with a spill stack
bool variant_quantized(int var);
// LDS stack entries of the trace kernel for a BVH4 needing need = depth + 1 entries
// (collapse_bvh4's bound; scenes needing more than 32 take the spill-stack global variant)
int stack_variant(int depth);
// bytes of the LDS-resident scene copy with its shading data (trace_kernel's, without the stacks)
size_t lds_scene_bytes(const LdsSizes& z);
// dynamic LDS of a launch of variant `var`: `stack` is the instantiation set's entries per lane, z.stack
// the pooled kernel's own (TraceParams::lds_stack), which that kernel takes instead
size_t trace_smem_bytes(int stack, int var, const LdsSizes& z);
// LDS-resident scene: the copy is small enough to sit beside the stacks, and node indices and leaf
// references fit the LDS kernels' 16-bit stack entries
bool lds_fits(const LdsSizes& z);
// the variants that traverse the scene's wide tree of lds_width() children: the LDS-resident reference
// kernels (pooled and phase-aligned); the MIS, global-scene, hit-query and feature kernels keep the BVH4
bool variant_takes_width(int var);
// The width rule: children per node of the tree the LDS-resident kernels traverse.  z8: the scene's sizes
// with its BVH8 (width 8; n_node_f4 = 0: the scene has none), need8 that tree's worst-case stack entries,
// knob PRT_LDS_WIDTH (4 or 8 force the width where the BVH8 can run at all; anything else: the default).
// 8 needs a BVH8 whose stack fits the pooled kernel's 32 entries and whose copy is LDS-resident; the
// default also asks that the pooled kernel's LDS still gives seven blocks per CU.
int lds_width(const LdsSizes& z8, int need8, int knob);
// the variant of a launch whose flags name none: need4 = the BVH4's worst-case stack entries (z.stack too),
// stack4 = its LDS stack instantiation set (0: too deep for one)
int choose_variant(const LdsSizes& z, int need4, int stack4, bool mis);

// Pinhole camera with an affine matrix (no aperture, last row (0,0,0,1), all finite):
// the kernels may use the exact gen_ray shortcut (TraceParams::cam_fast) ...
bool camera_is_fast(const float* cam);
// ... with its host-evaluated constant terms: the ray origin M (0,0,0,1) and rd.z * M[i][2]
void camera_terms(const float* cam, float cam_o[3], float cam_k[3]);

}  // namespace prt

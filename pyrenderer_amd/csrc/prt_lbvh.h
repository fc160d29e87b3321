// prt_lbvh.h — launch interface of the device build of a resident scene's trees (prt_lbvh.hip; prt_scene_rebuild
// in prt_scene.cpp enqueues it): a linear BVH (Karras 2012) over the triangles' Morton codes,
// emitted top-down as a four- or eight-wide tree one level per launch.  Plain device pointers in and out, every
// launch on the caller's stream; the boxes are then filled by prt_refit.h's launches.  Internal to libprt.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prt {

// One node of a level under construction: the sorted-slot range [a, b] it covers (b < a: no slot at all, the
// root of a scene without triangles), the inner node of the binary tree that covers it, and the traversal stack
// entries its strict ancestors can hold (emit_wide's anc).
struct LbvhItem { int32_t a, b, idx, anc; };

// bytes of the work area the rocPRIM calls below ask for at n slots (the largest of them)
hipError_t lbvh_temp_bytes(int64_t n, size_t* bytes);

// Stage 1.  cen[3 t ..] = (lo + hi) * 0.5f of triangle t's vertex bounds; cbox[0..3) / [3..6) = the minimum /
// maximum of the centroids; codes[t] = the 30-bit Morton code, 10 bits per axis (x the most significant of each
// triple) of min((int)((c - cmin) / (cmax - cmin) * 1024.0f), 1023), an axis of zero extent giving 0;
// ids[t] = t.  n >= 1.
hipError_t launch_lbvh_codes(const float* tri_v, int64_t n, float* cen, float* cbox, uint32_t* codes, uint32_t* ids,
                             void* temp, size_t temp_bytes, hipStream_t stream);
// Stage 2.  Stable sort of (codes, ids) by code: order[s] = the triangle of slot s, keys[s] = code << 32 | s.
hipError_t launch_lbvh_sort(const uint32_t* codes, const uint32_t* ids, int64_t n, uint32_t* codes_sorted,
                            int32_t* order, uint64_t* keys, void* temp, size_t temp_bytes, hipStream_t stream);
// Stage 3.  split[i] of the n - 1 inner nodes of the binary radix tree over the (distinct) keys: node i covers
// a range [a, b] with i = a or i = b, its children cover [a, split] (the inner node `split` when it holds more
// than one key) and [split + 1, b] (the inner node split + 1).  The root is node 0.  n >= 2.
hipError_t launch_lbvh_topology(const uint64_t* keys, int64_t n, int32_t* split, hipStream_t stream);
// items[0] = the root's item (0, n - 1, node 0, anc 0); *max_anc = 0
hipError_t launch_lbvh_root(LbvhItem* items, int64_t n, int32_t* max_anc, hipStream_t stream);
// Stage 4, one level of the tree of `width` (4 or 8): the n_items nodes items[base .. base + n_items) take as
// children the ranges reached after log2(width) binary splits, a range of at most max_leaf slots stopping as a
// leaf.  cnt[j] = inner children of node base + j, off = their exclusive scan with off[n_items] the total (the
// caller reads it to size the next level); the inner children become the items from next_base on, in node then
// child order; child0[base + j] = the node index of j's first inner child; *max_anc grows to the largest anc
// of the level.  cnt and off hold n_items + 1 words.  Items, child0 and the node arrays need room for n - 1
// nodes (one for n < 2) and no more, whatever split[] holds: the ranges of a tree are distinct, nested or
// disjoint, and hold two slots or more each (prt_plan.h lbvh_node_capacity); a level holds at most n / 2.
hipError_t launch_lbvh_level(int width, LbvhItem* items, int64_t base, int64_t n_items, int64_t next_base,
                             const int32_t* split, int max_leaf, int32_t* cnt, int32_t* off, int32_t* child0,
                             int32_t* max_anc, void* temp, size_t temp_bytes, hipStream_t stream);
// The n_nodes records of the finished tree (prt_internal.h Bvh4Host / Bvh8Host): child refs, leaf_ref(first,
// count) or the node index, children in slot order; every box inverted (lo = +inf, hi = -inf), empty slots'
// refs kEmptyRef, the unused words 0.  launch_refit_level then fills the live boxes.
hipError_t launch_lbvh_emit(int width, const LbvhItem* items, const int32_t* child0, int64_t n_nodes,
                            const int32_t* split, int max_leaf, float* nodes, hipStream_t stream);
// out[i] = i: a tree numbered level by level has the iota as its level list
hipError_t launch_lbvh_iota(int32_t* out, int64_t n, hipStream_t stream);

}  // namespace prt

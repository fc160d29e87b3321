#pragma once
// prt_device.h — the per-ray path-tracing hot path for CDNA4 (gfx950).
//
// One persistent kernel runs PathTracer.trace (reference core/tracing.py:116-155)
// for every (pixel, sample) work item of a tile set.  Each 64-lane wave owns a
// work queue (chunks pulled from one device counter, handed to idle lanes with
// __ballot / popcount ranks — path regeneration), and every loop iteration runs
// exactly ONE ray query per active lane: either a closest-hit extension ray or
// an any-hit NEE shadow ray.  Lanes therefore stay busy across paths of
// different length, and both query kinds share one traversal loop.
//
// Arithmetic contract (shared with oracle/prt_oracle.c):
//   f32, no FMA contraction (-ffp-contract=off and the pragma below),
//   correctly rounded '/' and sqrtf (hipcc default on gfx950), expressions in
//   the reference's left-to-right order, the PCG stream of DESIGN.md §RNG and
//   the minimax sin/cos of the concentric map.
// Closest hit = minimal (t, original triangle index); the BVH only prunes.
//
// The device code by role; every unit includes this umbrella (compiled once per (traversal stack, stats)
// instantiation set by prt_trace_inst.hip, in parallel, by prt_trace_pool.hip for the pooled kernel and
// by prt_kernels.hip for the hit-query, camera and reduction kernels):
//   prt_math.h      math, guards, RNG and sampling
//   prt_traverse.h  stacks and traversal
//   prt_shade.h     launch parameters, staging, the chunk claim and the shading pieces shared by the kernels
//   prt_trace.h     trace_kernel
//   prt_pool.h      trace_kernel_pool
//   prt_variants.h  launch / occupancy dispatch over the variant table (prt_variant_table.h)
#pragma clang fp contract(off)

#include "prt_math.h"
#include "prt_traverse.h"
#include "prt_shade.h"
#include "prt_trace.h"
#include "prt_pool.h"
#include "prt_variants.h"

// prt_variant_table.h — the trace-kernel variants that exist, as data: ids and one row each.  No device
// code: prt_plan.cpp reads it for the size-only launch decisions, prt_variants.h derives the launch and
// occupancy dispatch from the same rows.
#pragma once

namespace prt {

// trace kernel variants (selectable at run time through PRT_FLAG_VARIANT).  All run the
// while-while traversal (prt_traverse.h traverse_ww4) over the BVH4 — the LDS-resident reference
// kernels (1, 2, 6, 7, 8) over the scene's BVH8 instead where the width rule says so (prt_plan.h
// lds_width; one instantiation per width, no variant id of its own) — and give bit-identical images;
// the measured history of the variants this set replaced is in DESIGN.md §2.
constexpr int kVarLds = 1;         // LDS-resident scene, phase-aligned ext/shadow iterations, >= 7 waves/SIMD
                                   // (72 VGPRs: C2 4.40 -> 4.23 ms against the 6-wave build)
constexpr int kVarLdsAnyOcc = 2;   // ... no occupancy target (LDS scenes too large for 6 blocks per CU)
constexpr int kVarGlobal = 3;      // global scene: quantised 64-B nodes, LDS stack + global spill area,
                                   // suspended traversal tails, >= 6 waves/SIMD
// estimator variants: the reference's unused MIS direct lighting (PRT_FLAG_MIS_NEE)
constexpr int kVarLdsMis = 4;      // LDS scene, mixed schedule, >= 6 waves/SIMD
constexpr int kVarGlobalMis = 5;   // kVarGlobal + MIS
constexpr int kVarLds6 = 6;        // kVarLds built for >= 6 waves/SIMD (80 VGPRs): LDS scenes whose copy
                                   // fits six blocks per CU but not seven
constexpr int kVarLdsPool = 7;     // LDS-resident scene, block-pooled shadow queries (trace_kernel_pool),
                                   // >= 7 waves/SIMD; the LDS stack size is P.lds_stack
constexpr int kVarLdsPool6 = 8;    // kVarLdsPool built for >= 6 waves/SIMD (80 VGPRs)
constexpr int kVarFirst = 1;
constexpr int kVarLast = 8;
// ids 9-14 were the round-5 schedules of trace_kernel_pool that did not become the default (fused,
// packed leaf trips, split arrival; DESIGN.md §9, logs in profiles/r05/{fused,pack,split}/): removed
// in round 6, the C-ABI rejects them as unknown variants

// Scene placement, estimator, kernel and the occupancy target (min waves per SIMD) each variant is
// built for.
struct Variant { int id; bool lds, mis, pool; int wpe; };
constexpr Variant kVariants[] = {
    {kVarLds, true, false, false, 7},      {kVarLdsAnyOcc, true, false, false, 1},
    {kVarGlobal, false, false, false, 6},  {kVarLdsMis, true, true, false, 6},
    {kVarGlobalMis, false, true, false, 6}, {kVarLds6, true, false, false, 6},
    {kVarLdsPool, true, false, true, 7},   {kVarLdsPool6, true, false, true, 6},
};
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);
// the row of variant `var`, or null
constexpr const Variant* find_variant(int var) {
    for (int i = 0; i < kNumVariants; ++i)
        if (kVariants[i].id == var) return &kVariants[i];
    return nullptr;
}

}  // namespace prt

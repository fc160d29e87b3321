#pragma once
// prt_variants.h — the launch / occupancy dispatch derived from the table of trace-kernel variants
// (prt_variant_table.h kVariants).
#pragma clang fp contract(off)

#include <type_traits>

#include "prt_pool.h"
#include "prt_trace.h"

namespace prt {

// Which STACK instantiations a variant has.  The pool kernel's LDS stack size is a launch parameter
// (P.lds_stack): one instantiation, compiled in its own unit (prt_trace_pool.hip, other
// register-allocation flags) and reached through the 16-entry set.  Global scenes (LDS part of the spill
// stack): 4 (tests), 16, 32; LDS scenes: 10, 16, 32.
constexpr bool stack_exists(const Variant& v, int stack) {
    return v.pool ? stack == 16 : v.lds ? stack != 4 : (stack == 4 || stack == 16 || stack == 32);
}

// f(integral_constant<int, row>) for variant `var`, if it has a STACK instantiation; returns whether
template <int STACK, int I = 0, class F>
static bool with_variant(int var, F&& f) {
    if constexpr (I < kNumVariants) {
        if (kVariants[I].id != var) return with_variant<STACK, I + 1>(var, f);
        if constexpr (stack_exists(kVariants[I], STACK)) {
            f(std::integral_constant<int, I>{});
            return true;
        }
    }
    return false;
}

template <int STACK, bool STATS>
static hipError_t launch_var(const TraceParams& P, int var, int grid, size_t smem, hipStream_t stream) {
    hipError_t e = hipErrorInvalidValue;
    with_variant<STACK>(var, [&](auto row) {
        constexpr Variant v = kVariants[decltype(row)::value];
        if constexpr (v.pool) {
            e = launch_trace_pool(P, STATS, v.wpe, grid, smem, stream);
        } else {
            // the LDS reference kernels exist per tree width (prt_plan.h variant_takes_width)
            if constexpr (v.lds && !v.mis) {
                if (P.lds_width == 8) trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 8><<<grid, kBlock, smem, stream>>>(P);
                else trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 4><<<grid, kBlock, smem, stream>>>(P);
            } else {
                trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 4><<<grid, kBlock, smem, stream>>>(P);
            }
            e = hipGetLastError();
        }
    });
    return e;
}

template <int STACK, bool STATS>
static int occ_var(int var, int width, size_t smem) {
    int n = 0;
    with_variant<STACK>(var, [&](auto row) {
        constexpr Variant v = kVariants[decltype(row)::value];
        if constexpr (v.pool) {
            n = trace_occ_pool(STATS, v.wpe, width, smem);
        } else if constexpr (v.lds && !v.mis) {
            if (width == 8)
                (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &n, trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 8>, kBlock, smem);
            else
                (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &n, trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 4>, kBlock, smem);
        } else {
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_kernel<STACK, STATS, v.lds, v.mis, v.wpe, 4>,
                                                               kBlock, smem);
        }
    });
    return n;
}

}  // namespace prt

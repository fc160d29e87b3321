// prt_host.h — what the host units of libprt's C ABI (include/prt.h) share: the error text, the device
// buffer / guard types, a scene's device residency with its per-stream render contexts, and the few
// functions one unit calls in another.  prt_scene.cpp: BVH handles, scene creation, a scene's variant;
// prt_capi.cpp: everything that launches on one device; prt_multi.cpp: the RCCL gather.  The
// arithmetic that needs no GPU is in prt_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/prt.h"
#include "prt_kernels.h"
#include "prt_lbvh.h"
#include "prt_plan.h"
#include "prt_refit.h"

namespace prt {

extern thread_local std::string g_err;   // prt_last_error's text (prt_scene.cpp)
inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(PRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// stats words of a scene (include/prt.h PRT_DIAG_*: what the STATS builds write where)
constexpr int kStatWords = PRT_DIAG_WORDS;

// Device buffer owned by its holder: freed by release() or, at the latest, by the destructor (the
// per-call buffers of prt_trace_rays / prt_closest_hits / prt_hit_all are locals, freed on return
// after their stream has been synchronised; round 4 leaked them on every call).  Not copyable.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Work buffers of one render stream.  Renders enqueued on distinct streams may run
// concurrently (a frame's tail overlapping the next frame's start), so everything a
// launch writes lives here: tile origins, per-sample radiance and primary rays, the
// work counter + watchdog flag, the spill area and the host-output sums.
struct RenderCtx {
    hipStream_t stream = nullptr;
    DevBuf tiles, buf, rays, rays_o, work, acc, spill;
    std::vector<uint32_t> tile_host;   // tile origins of the last upload (== device copy in `tiles`)
    uint64_t last_use = 0;
};
constexpr size_t kMaxCtx = 8;
// work.p: [0] chunk counter; [kFaultOffset] traversal watchdog flag
constexpr size_t kFaultOffset = 32;
inline int* fault_flag(const DevBuf& work) { return (int*)((char*)work.p + kFaultOffset); }

// What prt_scene_update needs of a scene beyond its device buffers: kept on the host at creation (the tree's
// triangle order, each wide tree's nodes by level, and the arrays pack_scene reads that an update does not
// replace), and the device copies and work buffers that the first update allocates — a scene that is never
// updated holds none of them.
struct RefitState {
    std::vector<int32_t> order;               // BVH slot -> triangle
    std::vector<int32_t> level4, level8;      // node indices by level (prt_plan.h wide_levels)
    std::vector<int64_t> off4, off8;
    std::vector<int32_t> tri_mat, sph_mat, light_tri, light_off;
    std::vector<float> mat;
    bool resident = false;                    // the device buffers below are allocated and filled
    DevBuf d_order, d_level4, d_level8, d_bounds, d_tri_v;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    // the last update: host validation + pack, uploads, triangle records, tree levels, quantiser (ms)
    double ms[5] = {0, 0, 0, 0, 0};
};

// What prt_scene_rebuild keeps between calls: the device build's work arrays (prt_plan.h lbvh_scratch), which
// the first rebuild allocates and a later one of the same scene finds large enough, and the last build's
// report (include/prt.h prt_scene_rebuild_info).
struct RebuildState {
    DevBuf cen, cbox, codes, ids, codes_sorted, keys, split, items, child0, cnt, off, max_anc, temp;
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // host validation + pack, uploads, codes, sort, binary tree, wide emission (both widths, with the per-level
    // read-backs), triangle records + boxes, quantiser (ms)
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // four-wide nodes, depth, stack need; eight-wide nodes (0: none), depth, stack need; LDS width; slots
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t count = 0;                        // rebuilds so far
};

struct Scene {
    int device = 0;
    RefitState refit;
    RebuildState rebuild;
    int max_leaf = 4;                // env PRT_MAX_LEAF as read at creation: a rebuild's leaves hold as many
    int lds_width_knob = 0;          // env PRT_LDS_WIDTH as read at creation (prt_plan.h lds_width)
    int64_t n_tri = 0, n_nodes = 0;
    int32_t depth = 0;
    int n_light = 0, n_mat = 0, cus = 0;
    int blocks_per_cu = 0;           // of the default variant
    int occ[2 * (kVarLast + 1)] = {0};  // blocks/CU per (variant, stats) once queried (variant_occ)
    int n_lt = 0;                    // emitter triangles
    int64_t n_tri_f4 = 0;
    float direct_rgb[3] = {0.9f, 0.85f, 0.7f};
    DevBuf nodes4q;                  // quantised BVH4 (prt_internal.h)
    int64_t n_node4q_f4 = 0;
    DevBuf nodes4, tris, tri_nm, tri_frame, mats, light_v, light_off, sph, sph_mat;
    int64_t n_node4_f4 = 0;
    int stack4 = 0;                  // stack variant for the BVH4 (0 = BVH4 unusable)
    int need4 = 0;                   // worst-case BVH4 traversal stack entries
    // the BVH8 of an LDS-resident scene (prt_internal.h Bvh8Host; n_node8_f4 = 0: none), its worst-case stack
    // entries and stack variant, and the width the LDS reference kernels traverse (prt_plan.h lds_width; env
    // PRT_LDS_WIDTH read at scene creation)
    DevBuf nodes8;
    int64_t n_node8_f4 = 0;
    int need8 = 0, stack8 = 0;
    int lds_width = 4;
    int leaf_break = -1;             // env PRT_LEAF_BREAK (0..64); -1: per variant (trace launch)
    int leaf_exit = -1;              // env PRT_LEAF_EXIT (0..64); -1: per variant (trace launch)
    int resume_min = 32;             // resume variants (env PRT_RESUME_MIN; C4 after the r02 BVH fixes: 16 / 24 / 32 / 40 / 48 -> 19.4 / 19.1 / 19.0 / 19.4 / 19.8 ms)
    int pool_resume_min = 12;        // pooled kernel's extension-tail suspension (env PRT_POOL_RESUME_MIN, 0..64; 0: off;
                                     // C2 one-frame launches at 0 / 8 / 12 / 16 / 24: 3.89 / 3.62 / 3.61 / 3.61 / 3.63 ms,
                                     // profiles/r07/pool_resume/)
    uint32_t guard_trips = 1u << 20; // traversal phases per query before the watchdog trips (env PRT_GUARD_TRIPS)
    int spill_lds = 16;              // LDS part of the spill variants' stack (env PRT_SPILL_LDS: 4, 16 or 32)
    std::string wave_clock_path;     // env PRT_WAVE_CLOCK: append each trace launch's per-wave clocks here
    int64_t n_sph = 0;
    bool plain = false;              // no spheres, no metal / dielectric material (TraceParams::plain)
    bool shade_fast = false;         // TraceParams::shade_fast (prt_plan.h pack_scene)
    DevBuf work, stats;              // work: hit-query watchdog flag; stats: PRT_FLAG_STATS counters
    hipStream_t stream = nullptr;
    std::vector<std::unique_ptr<RenderCtx>> ctx;  // per render stream (<= kMaxCtx)
    uint64_t use_clock = 0;
    std::vector<hipEvent_t> ev;   // start/stop pairs of the last timed call
    int ev_used = 0;
    // per-sample buffer budget of one trace launch (radiance + primary rays): 16 GiB of the 288 GB
    // of HBM makes config 3 one launch per frame and config 5 eight (4 GiB: 2 and 29), +0.4 / +0.5 %
    // from the launch tails saved (profiles/r02/s5/chunk_ab/)
    size_t chunk_bytes = (size_t)16 << 30;
    size_t device_bytes = 0;
    // prt_render / prt_render_multi (as the root): [x][y] output frame, gathered tile sums
    // of every rank and their tile origins (host copy kept alive for the async upload)
    DevBuf frame, gather, gather_xy;
    std::vector<uint32_t> gather_xy_host;
    // prt_scatter_tiles: tile origins of the last upload (host copy alive until it has run, i.e.
    // until scatter_ev completes; re-uploaded only when a call's tile set differs)
    DevBuf scatter_xy;
    std::vector<uint32_t> scatter_xy_host;
    hipEvent_t scatter_ev = nullptr;
};

// ---- prt_scene.cpp: the scene part of a launch's parameters, and the variant choice
void scene_params(Scene* s, TraceParams& P);
int variant_width(const Scene* s, int var);           // children per node of the tree variant `var` traverses
int variant_need(const Scene* s, int var);            // ... and that tree's worst-case stack entries
LdsSizes scene_sizes(const Scene* s, int var);        // the scene's sizes as variant `var` lays them out in LDS
bool lds_fits4(const Scene* s, int var);
int launch_variant(const Scene* s, uint32_t flags);   // the flags' variant, or the scene's default
int variant_stack(const Scene* s, int var);
int variant_occ(Scene* s, int var, bool stats);       // blocks per CU (>= 1)

// ---- prt_capi.cpp (shared with prt_multi.cpp)
int check_render_args(Scene* s, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                      int n_tiles, int spp, int depth);
int render_ctx(Scene* s, hipStream_t stream, RenderCtx** cx);
int enqueue_render(Scene* s, RenderCtx* cx, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                   int n_tiles, int spp, int depth, uint64_t seed, uint32_t flags, float* d_acc,
                   int first_sample = 0, bool accumulate = false, int n_frames = 1, int frame_stride = 0,
                   int64_t out_pitch = 0);
int take_fault_at(const DevBuf& work);

}  // namespace prt

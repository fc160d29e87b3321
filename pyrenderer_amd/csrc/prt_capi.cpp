// prt_capi.cpp — everything of the C ABI that launches on one device: the render enqueue
// (camera_kernel -> trace_kernel -> reduce_kernel per sample chunk, all on one stream) behind the
// render entry points, ray and hit queries, the scatter, and timing / watchdog / stats read-back.
#include <cstdio>
#include <new>

#include "prt_host.h"

namespace prt {

int check_render_args(Scene* s, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                      int n_tiles, int spp, int depth) {
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    if (!cam) return fail(PRT_ERR_ARG, "cam is NULL");
    if (W < 2 || H < 2) return fail(PRT_ERR_ARG, "W and H must be >= 2 (u = (x + r) / (W - 1))");
    if (tw < 1 || th < 1 || (tw & (tw - 1)) || (th & (th - 1)) || (int64_t)tw * th < 64 || (int64_t)tw * th > (1 << 20))
        return fail(PRT_ERR_ARG, "tile width/height must be powers of two with 64 <= tw*th <= 2^20");
    if (W > 65535 || H > 65535) return fail(PRT_ERR_ARG, "frame larger than 65535 pixels per side");
    if (n_tiles < 0 || (n_tiles > 0 && !tile_ids)) return fail(PRT_ERR_ARG, "bad tile list");
    if (spp < 0 || depth < 0) return fail(PRT_ERR_ARG, "spp and depth must be >= 0");
    int tiles_x = (W + tw - 1) / tw, tiles_y = (H + th - 1) / th;
    for (int i = 0; i < n_tiles; ++i)
        if (tile_ids[i] < 0 || tile_ids[i] >= tiles_x * tiles_y)
            return fail(PRT_ERR_ARG, "tile id out of range: " + std::to_string(tile_ids[i]));
    if ((int64_t)n_tiles * tw * th >= ((int64_t)1 << 31)) return fail(PRT_ERR_ARG, "too many pixels in one call");
    return PRT_OK;
}

// Reads a watchdog flag and clears it once read, so every fault is reported exactly once:
// by the call whose launch raised it (host-output renders, hit queries), or by the first
// prt_check_faults / prt_kernel_timing after a device-output render.  A flag left set would
// otherwise be reported against every later, clean render (callers synchronise first).
int take_fault_at(const DevBuf& work) {
    int f = 0;
    if (!work.p) return 0;
    if (hipMemcpy(&f, fault_flag(work), sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (f != 0 && hipMemset(fault_flag(work), 0, sizeof(int)) != hipSuccess) return -1;
    return f;
}

// The render context of `stream` (null: the scene's), created on first use.  Beyond kMaxCtx streams
// the least recently used context is recycled after a device synchronisation.
int render_ctx(Scene* s, hipStream_t stream, RenderCtx** cx) {
    if (!stream) stream = s->stream;
    ++s->use_clock;
    using Ctx = std::unique_ptr<RenderCtx>;
    auto it = std::find_if(s->ctx.begin(), s->ctx.end(), [&](const Ctx& c) { return c->stream == stream; });
    if (it == s->ctx.end() && s->ctx.size() >= kMaxCtx) {
        it = std::min_element(s->ctx.begin(), s->ctx.end(),
                              [](const Ctx& a, const Ctx& b) { return a->last_use < b->last_use; });
        if (hipDeviceSynchronize() != hipSuccess) it = s->ctx.end();
    } else if (it == s->ctx.end()) {
        Ctx c(new (std::nothrow) RenderCtx());
        if (c && c->work.ensure(64) == hipSuccess && hipMemset(c->work.p, 0, 64) == hipSuccess) {
            s->ctx.push_back(std::move(c));
            it = s->ctx.end() - 1;
        }
    }
    if (it == s->ctx.end()) return fail(PRT_ERR_OOM, "render context allocation failed");
    (*it)->stream = stream;
    (*it)->last_use = s->use_clock;
    *cx = it->get();
    return PRT_OK;
}

namespace {

// every render context's watchdog flag (all are taken, not only the first one set)
int take_render_faults(Scene* s) {
    int any = 0;
    for (auto& c : s->ctx)
        if (int f = take_fault_at(c->work)) any = any ? any : f;
    return any;
}
// the report of a watchdog flag just taken
int watchdog_error(int fault) {
    return fault ? fail(PRT_ERR_INTERNAL, "traversal watchdog tripped (corrupt acceleration structure?)") : PRT_OK;
}

// the first n stats words of the last PRT_FLAG_STATS launch (words past kStatWords read 0)
int read_stats(Scene* s, uint64_t* out, int n) {
    unsigned long long h[kStatWords];
    const int k = std::min(n, kStatWords);
    if (k > 0) HIP_TRY(hipMemcpy(h, s->stats.p, sizeof(unsigned long long) * (size_t)k, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) out[i] = i < k ? h[i] : 0;
    return PRT_OK;
}

// Per-tile pixel origins of a context's launches, uploaded only when they differ from the context's
// last upload (a bench or animation re-renders the same tile set every frame), so a steady-state
// frame enqueues no host-to-device copy.  Enqueued on the context's stream, behind any render still
// running there (an unsynchronised prt_render_tiles_device reads the old origins until it ends); the
// source storage moves into cx->tile_host and lives until the next upload.
int upload_tiles(RenderCtx* cx, std::vector<uint32_t>& origins) {
    if (origins == cx->tile_host) return PRT_OK;
    HIP_TRY(cx->tiles.ensure(sizeof(uint32_t) * origins.size()));
    HIP_TRY(hipMemcpyAsync(cx->tiles.p, origins.data(), sizeof(uint32_t) * origins.size(), hipMemcpyHostToDevice,
                           cx->stream));
    cx->tile_host.swap(origins);
    return PRT_OK;
}

// blocks of a persistent launch: every resident block of the device, or fewer for a short queue
int persistent_grid(int occ, int cus, int64_t n_items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)occ * cus, (n_items + 255) / 256));
}

// Kernel variant (flags or the scene's default), its traversal stack, the blocks per CU of
// the persistent grid and the spill area of the global variants; switches P to the quantised
// nodes for the variants that read them.
struct TraceSetup { int var, stack, occ; };
int trace_setup(Scene* s, RenderCtx* cx, uint32_t flags, int64_t n_items, TraceParams& P, TraceSetup* out) {
    const bool stats = (flags & PRT_FLAG_STATS) != 0;
    const bool mis = (flags & PRT_FLAG_MIS_NEE) != 0;
    const int var = launch_variant(s, flags);
    if (var < kVarFirst || var > kVarLast) return fail(PRT_ERR_ARG, "unknown kernel variant");
    if (variant_mis(var) != mis)
        return fail(PRT_ERR_ARG, "PRT_FLAG_MIS_NEE must be set exactly for the MIS estimator variants");
    const bool spill = variant_spills(var);
    // the LDS reference kernels traverse the scene's tree of lds_width children (prt_plan.h), all others the BVH4
    const int width = variant_width(s, var), need = variant_need(s, var);
    if (variant_stack(s, var) == 0 && !spill) return fail(PRT_ERR_ARG, "BVH4 too deep for the LDS traversal stack variants");
    if (variant_quantized(var)) {
        P.nodes = (const float4*)s->nodes4q.p;
        P.n_node_f4 = (int)s->n_node4q_f4;
    } else if (width == 8) {
        P.nodes = (const float4*)s->nodes8.p;
        P.n_node_f4 = (int)s->n_node8_f4;
    }
    P.lds_width = width;
    const bool lds_var = variant_uses_lds(var);
    if (lds_var && !lds_fits4(s, var)) return fail(PRT_ERR_ARG, "scene too large for the LDS variant");
    if (variant_pool(var) && (need > 32 || need < 1))
        return fail(PRT_ERR_ARG, "BVH4 too deep for the pooled-shadow variant's LDS stack");
    // while-while leaf-phase entry: LDS scenes wait for every descending lane's leaf (their
    // leaves are cheap and traversals short); global scenes enter the leaf phase once at
    // most 16 descending lanes still lack one (C4: 35.1 -> 29.7 ms at 8 in round 1, 18.69 ->
    // 18.44 ms at 16 with leaf exit 12 after the round-2 traversal changes; C2 prefers 0).
    // Leaf-phase exit: back to descending once at most 8 (LDS) / 24 (global) lanes still
    // hold a leaf (C2 5.25 -> 5.04 ms in round 1, flat for 8-16 now; C4 with pixel-major
    // chunks 17.37-17.46 ms at 24 against 17.50-17.64 at 12 in three interleaved rounds,
    // profiles/r03/s1_baseline/leafexit/).  The eight-wide tree keeps 8: C2 3.506 / 3.377 / 3.376 / 3.385 /
    // 3.412 / 3.446 ms per launch at 0 / 4 / 6 / 8 / 10 / 12, and 3.504 at the 16 that the trip model
    // preferred (profiles/r13/lds_bvh8/)
    P.lds_stack = need;
    P.leaf_break = s->leaf_break >= 0 ? s->leaf_break : (lds_var ? 0 : 16);
    P.leaf_exit = s->leaf_exit >= 0 ? s->leaf_exit : (lds_var ? 8 : 24);
    const int occ = variant_occ(s, var, stats);
    // suspended extension tails pay only while finished lanes can be refilled: a launch with at most one
    // item per resident lane runs without them (a wave learns that the queue is empty only at its first
    // refill with an idle lane; C1's one-frame launches 0.096 vs 0.083 ms with the threshold left on)
    if (n_items <= (int64_t)occ * s->cus * 256) P.pool_resume_min = 0;
    if (spill) {
        // entries [spill_lds, need4] of every lane of the largest grid, plus one slot of headroom
        size_t per_lane = (size_t)std::max(1, s->need4 + 2 - s->spill_lds);
        HIP_TRY(cx->spill.ensure(per_lane * (size_t)occ * s->cus * 256 * sizeof(int)));
        P.spill = (int*)cx->spill.p;
    }
    *out = TraceSetup{var, variant_stack(s, var), occ};
    return PRT_OK;
}

void seed_params(TraceParams& P, uint64_t seed) { P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32); }

// Camera and frame part of a launch's parameters (camera_kernel's gen_ray inputs): the record, the
// pinhole shortcut's host-evaluated constant terms (TraceParams::cam_fast), resolution and tiling, the
// tile origins, and the keys of its samples: frames of spp samples, frame f's starting at first_sample
// + f * frame_stride (global_sample divides by frame_spp).
void frame_params(TraceParams& P, const float* cam, int W, int H, int tw, int th, const DevBuf& tiles, int64_t n_slots,
                  uint64_t seed, int first_sample, int spp, int frame_stride) {
    std::memcpy(P.cam, cam, sizeof(float) * PRT_CAM_FLOATS);
    P.cam_fast = camera_is_fast(cam) ? 1 : 0;
    camera_terms(cam, P.cam_o, P.cam_k);
    P.W = W; P.H = H;
    P.wm1 = (float)(W - 1); P.hm1 = (float)(H - 1);
    P.log_tw = __builtin_ctz((unsigned)tw);
    P.log_tpx = __builtin_ctz((unsigned)(tw * th));
    P.tile_xy = (const uint32_t*)tiles.p;
    P.n_slots = (int)n_slots;
    seed_params(P, seed);
    P.s0 = first_sample;
    P.frame_spp = (uint32_t)spp;
    P.frame_stride = (uint32_t)frame_stride;
}

}  // namespace

// Enqueue the whole render of a tile set on the context's stream, result in d_acc: samples
// first_sample .. first_sample + spp - 1 of every pixel; `accumulate` adds them onto the
// sums already in d_acc (progressive rendering) instead of overwriting them.
// n_frames > 1 (prt_render_frames_device): frame f renders samples first_sample + f * frame_stride
// + 0 .. spp - 1 into d_acc + f * out_pitch floats (0: packed, n_slots * 3), and all frames' items run
// through the same persistent launches (a launch covers up to the memory budget's worth of frames),
// so the launch drains once per launch instead of once per frame.
int enqueue_render(Scene* s, RenderCtx* cx, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                   int n_tiles, int spp, int depth, uint64_t seed, uint32_t flags, float* d_acc, int first_sample,
                   bool accumulate, int n_frames, int frame_stride, int64_t out_pitch) {
    if (flags & PRT_FLAG_NO_PRIMARY_KERNEL)
        return fail(PRT_ERR_UNSUP, "PRT_FLAG_NO_PRIMARY_KERNEL: camera rays always come from the camera kernel "
                                   "(the trace kernels no longer carry camera code)");
    const int64_t n_slots = (int64_t)n_tiles * tw * th;
    if (n_slots == 0) return PRT_OK;
    if (out_pitch == 0) out_pitch = 3 * n_slots;
    hipStream_t stream = cx->stream;
    std::vector<uint32_t> origins = tile_origins(tile_ids, n_tiles, (W + tw - 1) / tw, tw, th);
    if (int rc = upload_tiles(cx, origins)) return rc;
    if (spp == 0 || depth == 0) {
        // every sample's radiance is 0: the sums are 0, or unchanged when accumulating
        if (!accumulate)
            HIP_TRY(hipMemset2DAsync(d_acc, sizeof(float) * (size_t)out_pitch, 0, sizeof(float) * 3 * (size_t)n_slots,
                                     (size_t)n_frames, stream));
        return PRT_OK;
    }
    // the launches' sample space: j = f * spp + (sample of frame f), T of them
    const int64_t T = (int64_t)spp * n_frames;
    // per-sample buffers: radiance (12 B) + primary ray (16 B) + its origin (16 B, cameras other than
    // the affine pinhole, whose origin is uniform)
    const bool cam_fast = camera_is_fast(cam);
    int64_t per_sample = n_slots * 3 * (int64_t)sizeof(float);
    int64_t per_sample_all = per_sample + n_slots * (cam_fast ? 16 : 32);
    // per-launch budget: the scene's (<= 16 GiB), and when this context's buffers must grow, at
    // most half of the device memory free now plus what they already hold — every render stream
    // (up to kMaxCtx) owns such a buffer set, so a budget fixed at scene creation could ask
    // several streams' worth of the memory that was free then
    size_t budget = s->chunk_bytes;
    {
        const size_t held = cx->buf.bytes + cx->rays.bytes + cx->rays_o.bytes;
        size_t free_b = 0, total_b = 0;
        if ((size_t)(std::min<int64_t>(T, (int64_t)(budget / (size_t)per_sample_all)) * per_sample_all) > held &&
            hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
            budget = std::min(budget, std::max<size_t>((size_t)per_sample_all, (free_b + held) / 2));
    }
    const ChunkPlan plan = plan_chunks(T, n_slots, per_sample_all, budget);
    const int64_t chunk = plan.chunk;
    HIP_TRY(cx->buf.ensure((size_t)(chunk * per_sample)));
    HIP_TRY(cx->rays.ensure((size_t)(chunk * n_slots * 16)));
    if (!cam_fast) HIP_TRY(cx->rays_o.ensure((size_t)(chunk * n_slots * 16)));
    const bool stats = (flags & PRT_FLAG_STATS) != 0;
    const bool timed = (flags & PRT_FLAG_TIME) != 0;
    if (stats) HIP_TRY(hipMemsetAsync(s->stats.p, 0, kStatWords * sizeof(unsigned long long), stream));

    TraceParams P;
    scene_params(s, P);
    frame_params(P, cam, W, H, tw, th, cx->tiles, n_slots, seed, first_sample, spp, frame_stride);
    P.rays = (const float4*)cx->rays.p;
    P.ray_o = cam_fast ? nullptr : (const float4*)cx->rays_o.p;
    P.depth = depth;
    P.work = (uint32_t*)cx->work.p;
    P.fault = fault_flag(cx->work);
    P.out = (float*)cx->buf.p;
    TraceSetup ts;
    if (int rc = trace_setup(s, cx, flags, chunk * n_slots, P, &ts)) return rc;
    // timed launches accumulate event pairs until prt_kernel_timing() reads them
    int k = s->ev_used / 2;
    if (timed) {
        while ((int64_t)s->ev.size() < s->ev_used + 2 * plan.n_launches) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            s->ev.push_back(e);
        }
        s->ev_used += (int)(2 * plan.n_launches);
    }
    for (int64_t s0 = 0; s0 < T; s0 += chunk, ++k) {
        int64_t n = std::min<int64_t>(chunk, T - s0);
        P.j0 = (uint32_t)s0;   // launch sample offset: keys the RNG streams through global_sample()
        P.n_items = (uint64_t)(n * n_slots);
        const int grid = persistent_grid(ts.occ, s->cus, (int64_t)P.n_items);
        // the camera kernel also zeroes the work counter (and, for the first chunk, the watchdog
        // flag) ahead of the trace launch: two fewer stream operations per frame
        P.cam_clears = 1 | (s0 == 0 ? 2 : 0);
        HIP_TRY(launch_camera(P, (float4*)cx->rays.p, cam_fast ? nullptr : (float4*)cx->rays_o.p, stream));
        P.cam_clears = 0;
        if (timed) HIP_TRY(hipEventRecord(s->ev[2 * k], stream));
        DevBuf wclk;
        if (!s->wave_clock_path.empty()) {
            HIP_TRY(wclk.ensure(sizeof(unsigned long long) * 3 * (size_t)grid * (256 / 64)));
            HIP_TRY(hipMemsetAsync(wclk.p, 0, sizeof(unsigned long long) * 3 * (size_t)grid * 4, stream));
            P.wave_clock = (unsigned long long*)wclk.p;
        }
        HIP_TRY(launch_trace(P, ts.stack, ts.var, grid, stats, stream));
        if (timed) HIP_TRY(hipEventRecord(s->ev[2 * k + 1], stream));
        if (P.wave_clock) {
            // diagnostic only: synchronous read-back, appended as (start, end, items) u64 triples
            std::vector<unsigned long long> h((size_t)grid * 4 * 3);
            HIP_TRY(hipMemcpyAsync(h.data(), wclk.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost,
                                   stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (FILE* f = std::fopen(s->wave_clock_path.c_str(), "ab")) {
                std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
                std::fclose(f);
            }
            P.wave_clock = nullptr;
        }
        // every frame overlapping the chunk, one launch: frame f sums its samples of [s0, s0 + n) in order
        const FrameSpan fs = launch_frames(s0, n, spp, n_frames);
        for (int64_t fa = fs.f0; fa < fs.f1; fa += 65535)
            HIP_TRY(launch_reduce((const float*)cx->buf.p, d_acc, (int)n_slots, s0, n, spp, fa,
                                  std::min<int64_t>(65535, fs.f1 - fa), out_pitch, accumulate, stream));
    }
    return PRT_OK;
}

namespace {

// host-output tail of a render on the scene's stream: wait, report the watchdog, return the counters
int finish_render(Scene* s, RenderCtx* cx, uint32_t flags, uint64_t* stats) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (int rc = watchdog_error(take_fault_at(cx->work))) return rc;
    if (!stats) return PRT_OK;
    if (flags & PRT_FLAG_STATS) return read_stats(s, stats, 4);
    std::memset(stats, 0, 4 * sizeof(uint64_t));
    return PRT_OK;
}

// front half of the hit queries: the scene's parameters, the rays on the device, one launch_hits
struct HitBufs { DevBuf rays, id, t; };
int enqueue_hits(Scene* s, const float* rays, int64_t n, bool quant, bool any, TraceParams& P, HitBufs& b) {
    scene_params(s, P);
    if (quant) P.nodes = (const float4*)s->nodes4q.p;
    P.fault = fault_flag(s->work);
    HIP_TRY(b.rays.ensure(sizeof(float) * 8 * (size_t)n));
    HIP_TRY(b.id.ensure(sizeof(int32_t) * (size_t)n));
    HIP_TRY(b.t.ensure(sizeof(float) * (size_t)n));
    HIP_TRY(hipMemsetAsync(P.fault, 0, sizeof(int), s->stream));
    HIP_TRY(hipMemcpyAsync(b.rays.p, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(launch_hits(P, quant, any, 64, (const float4*)b.rays.p, n, (int*)b.id.p, (float*)b.t.p, s->stream));
    return PRT_OK;
}

// prt_features / prt_features_device: the argument checks, before any device call
int check_features_args(Scene* s, const float* cam, int W, int H, int first_sample, int samples, uint32_t flags,
                        const float* out) {
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    if (!cam) return fail(PRT_ERR_ARG, "cam is NULL");
    if (!out) return fail(PRT_ERR_ARG, "out is NULL");
    if (W < 1 || H < 1) return fail(PRT_ERR_ARG, "W and H must be >= 1");
    if (W > 65535 || H > 65535) return fail(PRT_ERR_ARG, "frame larger than 65535 pixels per side");
    if (samples < 1) return fail(PRT_ERR_ARG, "samples must be >= 1");
    if (first_sample < 0 || (int64_t)first_sample + samples > INT32_MAX)
        return fail(PRT_ERR_ARG, "first_sample must be >= 0 and first_sample + samples < 2^31");
    if (flags & ~PRT_HITS_QUANTIZED) return fail(PRT_ERR_ARG, "prt_features takes only PRT_HITS_QUANTIZED");
    if (s->need4 > 64) return fail(PRT_ERR_ARG, "BVH4 too deep for the hit-query kernel");
    return PRT_OK;
}

// ... and the one launch: the camera and sample keys as prt_camera_rays sets them (frame_params: one frame
// of `samples` samples from first_sample), the traversal stack sized to the scene's own bound
int enqueue_features(Scene* s, const float* cam, int W, int H, int first_sample, int samples, uint64_t seed,
                     uint32_t flags, int* fault, float* d_out, hipStream_t stream) {
    const bool quant = (flags & PRT_HITS_QUANTIZED) != 0;
    TraceParams P;
    scene_params(s, P);
    if (quant) P.nodes = (const float4*)s->nodes4q.p;
    frame_params(P, cam, W, H, 8, 8, DevBuf(), 0, seed, first_sample, samples, 0);   // no tiles: one lane per pixel
    P.fault = fault;
    HIP_TRY(launch_features(P, quant, std::max(s->need4, 4), samples, d_out, stream));
    return PRT_OK;
}

// a device-wide self-test kernel's n counters
int selftest(int device, uint64_t* out, int n, hipError_t (*launch)(unsigned long long*, hipStream_t)) {
    if (!out) return fail(PRT_ERR_ARG, "NULL argument");
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(PRT_ERR_HIP, "no such HIP device");
    DeviceGuard g(device);
    DevBuf d;
    unsigned long long h[16];
    HIP_TRY(d.ensure(n * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(d.p, 0, n * sizeof(unsigned long long)));
    HIP_TRY(launch((unsigned long long*)d.p, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h, d.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) out[i] = h[i];
    return PRT_OK;
}

// stats read-back entry points: the device idle, then the first n words
int synced_stats(void* scene, uint64_t* out, int n, const char* bad_args) {
    auto* s = (Scene*)scene;
    if (!s || !out || n < 0) return fail(PRT_ERR_ARG, bad_args);
    DeviceGuard g(s->device);
    HIP_TRY(hipDeviceSynchronize());
    return read_stats(s, out, n);
}

}  // namespace
}  // namespace prt

using namespace prt;

extern "C" {

int prt_closest_hits(void* scene, const float* rays, int64_t n, uint32_t flags, int32_t* hit_id, float* hit_t) {
    auto* s = (Scene*)scene;
    if (!s || (n > 0 && (!rays || !hit_id || !hit_t))) return fail(PRT_ERR_ARG, "NULL argument");
    if (n < 0) return fail(PRT_ERR_ARG, "n < 0");
    if (n == 0) return PRT_OK;
    if (s->need4 > 64) return fail(PRT_ERR_ARG, "BVH4 too deep for the hit-query kernel");
    DeviceGuard g(s->device);
    TraceParams P;
    HitBufs b;
    if (int rc = enqueue_hits(s, rays, n, (flags & PRT_HITS_QUANTIZED) != 0, (flags & PRT_HITS_ANY) != 0, P, b)) return rc;
    HIP_TRY(hipMemcpyAsync(hit_id, b.id.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(hit_t, b.t.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return watchdog_error(take_fault_at(s->work));
}

int prt_hit_all(void* scene, const float* rays, int64_t n, uint64_t seed, uint32_t flags, float* out16) {
    auto* s = (Scene*)scene;
    if (!s || (n > 0 && (!rays || !out16))) return fail(PRT_ERR_ARG, "NULL argument");
    if (n < 0) return fail(PRT_ERR_ARG, "n < 0");
    if (flags & ~PRT_HITS_QUANTIZED) return fail(PRT_ERR_ARG, "prt_hit_all takes only PRT_HITS_QUANTIZED");
    if (n == 0) return PRT_OK;
    if (s->need4 > 64) return fail(PRT_ERR_ARG, "BVH4 too deep for the hit-query kernel");
    DeviceGuard g(s->device);
    TraceParams P;
    HitBufs b;
    DevBuf d_out;
    HIP_TRY(d_out.ensure(sizeof(float) * 16 * (size_t)n));
    if (int rc = enqueue_hits(s, rays, n, (flags & PRT_HITS_QUANTIZED) != 0, false, P, b)) return rc;
    seed_params(P, seed);
    HIP_TRY(launch_hit_shade(P, (const float4*)b.rays.p, n, (const int*)b.id.p, (const float*)b.t.p, (float*)d_out.p,
                             s->stream));
    HIP_TRY(hipMemcpyAsync(out16, d_out.p, sizeof(float) * 16 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return watchdog_error(take_fault_at(s->work));
}

int prt_trace_rays(void* scene, const float* rays, int64_t n, int depth, uint64_t seed, uint32_t flags,
                   float* out_rgb) {
    auto* s = (Scene*)scene;
    if (!s || (n > 0 && (!rays || !out_rgb))) return fail(PRT_ERR_ARG, "NULL argument");
    if (n < 0 || depth < 0) return fail(PRT_ERR_ARG, "n and depth must be >= 0");
    if (flags & (PRT_FLAG_NO_PRIMARY_KERNEL | PRT_FLAG_TIME))
        return fail(PRT_ERR_ARG, "prt_trace_rays: PRT_FLAG_NO_PRIMARY_KERNEL / PRT_FLAG_TIME do not apply");
    if (n == 0) return PRT_OK;
    if (n >= ((int64_t)1 << 31)) return fail(PRT_ERR_ARG, "too many rays in one call (< 2^31)");
    DeviceGuard g(s->device);
    if (depth == 0) {
        std::memset(out_rgb, 0, sizeof(float) * 3 * (size_t)n);
        return PRT_OK;
    }
    RenderCtx* cx;
    if (int rc = render_ctx(s, s->stream, &cx)) return rc;
    // the rays as one "sample" of a frame of 64 x 1 tiles: item = slot = ray index (every chunk
    // of 64 items one tile); the trace kernel's tile origins are (0, tile)
    constexpr int64_t kRowRays = 64;
    const int64_t n_pad = (n + kRowRays - 1) / kRowRays * kRowRays;
    const int64_t n_tiles = n_pad / kRowRays;
    if (n_tiles > 65535) return fail(PRT_ERR_ARG, "too many rays in one call (<= 65535 x 64)");
    std::vector<uint32_t> origins((size_t)n_tiles);
    for (int64_t t = 0; t < n_tiles; ++t) origins[(size_t)t] = (uint32_t)t;
    if (int rc = upload_tiles(cx, origins)) return rc;
    DevBuf d_in, d_org, d_out;
    HIP_TRY(d_in.ensure(sizeof(float) * 8 * (size_t)n));
    HIP_TRY(d_org.ensure(sizeof(float) * 4 * (size_t)n_pad));
    HIP_TRY(d_out.ensure(sizeof(float) * 3 * (size_t)n_pad));
    HIP_TRY(cx->rays.ensure(sizeof(float) * 4 * (size_t)n_pad));
    HIP_TRY(hipMemcpyAsync(d_in.p, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    TraceParams P;
    scene_params(s, P);
    P.rays = (const float4*)cx->rays.p;
    P.ray_o = (const float4*)d_org.p;
    P.W = (int)kRowRays; P.H = (int)n_tiles;
    P.wm1 = (float)(kRowRays - 1); P.hm1 = (float)std::max<int64_t>(n_tiles - 1, 1);
    P.log_tw = 6; P.log_tpx = 6;
    P.tile_xy = (const uint32_t*)cx->tiles.p;
    P.n_slots = (int)n_pad; P.n_items = (uint64_t)n_pad;
    P.depth = depth;
    seed_params(P, seed);
    P.work = (uint32_t*)cx->work.p;
    P.fault = fault_flag(cx->work);
    P.out = (float*)d_out.p;
    TraceSetup ts;
    if (int rc = trace_setup(s, cx, flags, n_pad, P, &ts)) return rc;
    const bool stats = (flags & PRT_FLAG_STATS) != 0;
    if (stats) HIP_TRY(hipMemsetAsync(s->stats.p, 0, kStatWords * sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemsetAsync(cx->work.p, 0, 64, s->stream));   // work counter and watchdog flag
    HIP_TRY(launch_rays_prep(P, (const float*)d_in.p, n, n_pad, (float4*)cx->rays.p, (float4*)d_org.p, s->stream));
    HIP_TRY(launch_trace(P, ts.stack, ts.var, persistent_grid(ts.occ, s->cus, n_pad), stats, s->stream));
    HIP_TRY(hipMemcpyAsync(out_rgb, d_out.p, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return watchdog_error(take_fault_at(cx->work));
}

int prt_camera_rays(void* scene, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                    int n_tiles, int first_sample, int spp, uint64_t seed, float* out8) {
    auto* s = (Scene*)scene;
    if (int rc = check_render_args(s, cam, W, H, tw, th, tile_ids, n_tiles, spp, 1)) return rc;
    if (first_sample < 0 || (int64_t)first_sample + spp > INT32_MAX)
        return fail(PRT_ERR_ARG, "sample indices must stay in [0, 2^31)");
    const int64_t n_slots = (int64_t)n_tiles * tw * th, n = n_slots * spp;
    if (n == 0) return PRT_OK;
    if (!out8) return fail(PRT_ERR_ARG, "out8 is NULL");
    if (n >= ((int64_t)1 << 31)) return fail(PRT_ERR_ARG, "too many rays in one call (< 2^31)");
    DeviceGuard g(s->device);
    // a tile buffer of its own: a render context's cached upload stays as it is
    const std::vector<uint32_t> origins = tile_origins(tile_ids, n_tiles, (W + tw - 1) / tw, tw, th);
    DevBuf d_tiles, d_rays, d_org;
    HIP_TRY(d_tiles.ensure(sizeof(uint32_t) * (size_t)n_tiles));
    HIP_TRY(d_rays.ensure(16 * (size_t)n));
    HIP_TRY(d_org.ensure(16 * (size_t)n));
    HIP_TRY(hipMemcpyAsync(d_tiles.p, origins.data(), sizeof(uint32_t) * (size_t)n_tiles, hipMemcpyHostToDevice,
                           s->stream));
    TraceParams P;
    scene_params(s, P);
    // one frame of spp samples starting at first_sample, as enqueue_render keys it
    frame_params(P, cam, W, H, tw, th, d_tiles, n_slots, seed, first_sample, spp, 0);
    P.n_items = (uint64_t)n;   // one launch: j0 = 0, and the camera kernel clears nothing (cam_clears = 0)
    // slots outside the frame (partial edge tiles) get no ray from the camera kernel: their rows are
    // returned as zeros, not as uninitialised device memory
    HIP_TRY(hipMemsetAsync(d_rays.p, 0, 16 * (size_t)n, s->stream));
    if (!P.cam_fast) HIP_TRY(hipMemsetAsync(d_org.p, 0, 16 * (size_t)n, s->stream));
    HIP_TRY(launch_camera(P, (float4*)d_rays.p, P.cam_fast ? nullptr : (float4*)d_org.p, s->stream));
    std::vector<float> r((size_t)n * 4), o(P.cam_fast ? 0 : (size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(r.data(), d_rays.p, 16 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (!P.cam_fast) HIP_TRY(hipMemcpyAsync(o.data(), d_org.p, 16 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int64_t i = 0; i < n; ++i) {
        float* q = out8 + 8 * i;
        const bool in_frame = slot_in_frame(origins, i % n_slots, tw, th, W, H);
        for (int k = 0; k < 3; ++k) {
            q[k] = !in_frame ? 0.0f : P.cam_fast ? P.cam_o[k] : o[(size_t)(4 * i + k)];
            q[4 + k] = r[(size_t)(4 * i + k)];
        }
        q[3] = r[(size_t)(4 * i + 3)];   // the RNG state after the camera's draws (u32 bits)
        q[7] = 0.0f;
    }
    return PRT_OK;
}

int prt_features(void* scene, const float* cam, int W, int H, int first_sample, int samples, uint64_t seed,
                 uint32_t flags, float* out) {
    auto* s = (Scene*)scene;
    if (int rc = check_features_args(s, cam, W, H, first_sample, samples, flags, out)) return rc;
    DeviceGuard g(s->device);
    const size_t bytes = sizeof(float) * PRT_FEATURE_CHANNELS * (size_t)W * (size_t)H;
    DevBuf d_out;
    HIP_TRY(d_out.ensure(bytes));
    HIP_TRY(hipMemsetAsync(fault_flag(s->work), 0, sizeof(int), s->stream));
    if (int rc = enqueue_features(s, cam, W, H, first_sample, samples, seed, flags, fault_flag(s->work), (float*)d_out.p,
                                  s->stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return watchdog_error(take_fault_at(s->work));
}

int prt_features_device(void* scene, const float* cam, int W, int H, int first_sample, int samples, uint64_t seed,
                        uint32_t flags, float* d_out, void* stream) {
    auto* s = (Scene*)scene;
    if (int rc = check_features_args(s, cam, W, H, first_sample, samples, flags, d_out)) return rc;
    if ((uintptr_t)d_out & 15) return fail(PRT_ERR_ARG, "d_out must be 16-byte aligned");
    DeviceGuard g(s->device);
    // the watchdog flag of the stream's render context: a trip is reported by prt_check_faults
    RenderCtx* cx;
    if (int rc = render_ctx(s, (hipStream_t)stream, &cx)) return rc;
    return enqueue_features(s, cam, W, H, first_sample, samples, seed, flags, fault_flag(cx->work), d_out,
                            (hipStream_t)stream);
}

int prt_render_tiles(void* scene, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids, int n_tiles,
                     int spp, int depth, uint64_t seed, uint32_t flags, float* out_sum, uint64_t* stats) {
    auto* s = (Scene*)scene;
    if (int rc = check_render_args(s, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth)) return rc;
    if (!out_sum) return fail(PRT_ERR_ARG, "out_sum is NULL");
    DeviceGuard g(s->device);
    const int64_t n_slots = (int64_t)n_tiles * tw * th;
    RenderCtx* cx;
    if (int rc = render_ctx(s, s->stream, &cx)) return rc;
    HIP_TRY(cx->acc.ensure(std::max<size_t>(16, sizeof(float) * 3 * (size_t)n_slots)));
    if (int rc = enqueue_render(s, cx, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth, seed, flags, (float*)cx->acc.p))
        return rc;
    if (n_slots)
        HIP_TRY(hipMemcpyAsync(out_sum, cx->acc.p, sizeof(float) * 3 * (size_t)n_slots, hipMemcpyDeviceToHost, s->stream));
    return finish_render(s, cx, flags, stats);
}

int prt_render_tiles_accumulate(void* scene, const float* cam, int W, int H, int tw, int th,
                                const int32_t* tile_ids, int n_tiles, int first_sample, int spp, int depth,
                                uint64_t seed, uint32_t flags, float* io_sum) {
    auto* s = (Scene*)scene;
    if (int rc = check_render_args(s, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth)) return rc;
    if (!io_sum && n_tiles > 0) return fail(PRT_ERR_ARG, "io_sum is NULL");
    if (first_sample < 0 || (int64_t)first_sample + spp > INT32_MAX)
        return fail(PRT_ERR_ARG, "first_sample must be >= 0 and first_sample + spp < 2^31");
    DeviceGuard g(s->device);
    const int64_t n_slots = (int64_t)n_tiles * tw * th;
    if (n_slots == 0) return PRT_OK;
    RenderCtx* cx;
    if (int rc = render_ctx(s, s->stream, &cx)) return rc;
    const size_t bytes = sizeof(float) * 3 * (size_t)n_slots;
    HIP_TRY(cx->acc.ensure(std::max<size_t>(16, bytes)));
    HIP_TRY(hipMemcpyAsync(cx->acc.p, io_sum, bytes, hipMemcpyHostToDevice, s->stream));
    if (int rc = enqueue_render(s, cx, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth, seed, flags, (float*)cx->acc.p,
                                first_sample, true))
        return rc;
    HIP_TRY(hipMemcpyAsync(io_sum, cx->acc.p, bytes, hipMemcpyDeviceToHost, s->stream));
    return finish_render(s, cx, flags, nullptr);
}

int prt_render_tiles_device(void* scene, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                            int n_tiles, int spp, int depth, uint64_t seed, uint32_t flags, float* d_out_sum,
                            void* stream) {
    auto* s = (Scene*)scene;
    if (int rc = check_render_args(s, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth)) return rc;
    if (!d_out_sum && n_tiles > 0) return fail(PRT_ERR_ARG, "d_out_sum is NULL");
    DeviceGuard g(s->device);
    RenderCtx* cx;
    if (int rc = render_ctx(s, (hipStream_t)stream, &cx)) return rc;
    return enqueue_render(s, cx, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth, seed, flags, d_out_sum);
}

int prt_render_frames_device(void* scene, const float* cam, int W, int H, int tw, int th, const int32_t* tile_ids,
                             int n_tiles, int spp, int depth, uint64_t seed, int n_frames, int frame_stride,
                             uint32_t flags, float* d_out_sums, int64_t out_pitch, void* stream) {
    auto* s = (Scene*)scene;
    if (int rc = check_render_args(s, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth)) return rc;
    if (n_frames < 1) return fail(PRT_ERR_ARG, "n_frames must be >= 1");
    if (frame_stride < 0) return fail(PRT_ERR_ARG, "frame_stride must be >= 0");
    if ((int64_t)(n_frames - 1) * frame_stride + spp > INT32_MAX || (int64_t)n_frames * spp > INT32_MAX)
        return fail(PRT_ERR_ARG, "sample indices must stay below 2^31");
    if (!d_out_sums && n_tiles > 0) return fail(PRT_ERR_ARG, "d_out_sums is NULL");
    if (out_pitch != 0 && out_pitch < 3 * (int64_t)n_tiles * tw * th)
        return fail(PRT_ERR_ARG, "out_pitch must be 0 (packed frames) or >= n_tiles * tw * th * 3 floats");
    DeviceGuard g(s->device);
    RenderCtx* cx;
    if (int rc = render_ctx(s, (hipStream_t)stream, &cx)) return rc;
    return enqueue_render(s, cx, cam, W, H, tw, th, tile_ids, n_tiles, spp, depth, seed, flags, d_out_sums, 0, false,
                          n_frames, frame_stride, out_pitch);
}

int prt_kernel_timing(void* scene, double* ms_total, int64_t* launches) {
    auto* s = (Scene*)scene;
    if (!s || !ms_total || !launches) return fail(PRT_ERR_ARG, "NULL argument");
    DeviceGuard g(s->device);
    double tot = 0.0;
    for (int k = 0; k + 1 < s->ev_used; k += 2) {
        HIP_TRY(hipEventSynchronize(s->ev[k + 1]));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev[k], s->ev[k + 1]));
        tot += ms;
    }
    *ms_total = tot;
    *launches = s->ev_used / 2;
    s->ev_used = 0;
    return watchdog_error(take_render_faults(s));
}

int prt_selftest_guards(int device, uint64_t* counts16) { return selftest(device, counts16, 16, launch_guard_selftest); }

int prt_selftest_rcp(int device, uint64_t* mismatches8) { return selftest(device, mismatches8, 8, launch_rcp_selftest); }

int prt_check_faults(void* scene) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "NULL argument");
    DeviceGuard g(s->device);
    // every stream a render was enqueued on: the device-wide synchronisation also covers
    // streams the caller owns (torch streams) without holding their handles past their life
    HIP_TRY(hipDeviceSynchronize());
    return watchdog_error(take_render_faults(s) | take_fault_at(s->work));
}

int prt_last_stats(void* scene, uint64_t* stats4) { return synced_stats(scene, stats4, 4, "NULL argument"); }

int prt_diag_words(void* scene, uint64_t* out, int n) { return synced_stats(scene, out, n, "NULL argument or n < 0"); }

int prt_diag_stats(void* scene, uint64_t* stats16) { return synced_stats(scene, stats16, 16, "NULL argument"); }

int prt_render(void* scene, const float* cam, int W, int H, int x0, int y0, int w, int h, int spp, int depth,
               uint64_t seed, uint32_t flags, float* out_sum, uint64_t* stats) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || (int64_t)x0 + w > W || (int64_t)y0 + h > H)
        return fail(PRT_ERR_ARG, "window [x0, x0+w) x [y0, y0+h) must be non-empty and inside the W x H frame");
    if (!out_sum) return fail(PRT_ERR_ARG, "out_sum is NULL");
    // 8 x 8 tiles: one wave's 64 work items cover one square tile (coherent rays), and a
    // window wastes at most a 7-pixel border of its edge tiles
    constexpr int kT = 8;
    const std::vector<int32_t> ids = window_tiles(W, x0, y0, w, h, kT, kT);
    if (int rc = check_render_args(s, cam, W, H, kT, kT, ids.data(), (int)ids.size(), spp, depth)) return rc;
    DeviceGuard g(s->device);
    const int64_t n_slots = (int64_t)ids.size() * kT * kT;
    RenderCtx* cx;
    if (int rc = render_ctx(s, s->stream, &cx)) return rc;
    HIP_TRY(cx->acc.ensure(sizeof(float) * 3 * (size_t)n_slots));
    const size_t out_bytes = sizeof(float) * 3 * (size_t)w * (size_t)h;
    HIP_TRY(s->frame.ensure(out_bytes));
    if (int rc = enqueue_render(s, cx, cam, W, H, kT, kT, ids.data(), (int)ids.size(), spp, depth, seed, flags,
                                (float*)cx->acc.p))
        return rc;
    HIP_TRY(launch_scatter((const float*)cx->acc.p, (const uint32_t*)cx->tiles.p, (int)n_slots, 3, 6, x0, y0, w, h,
                           (float*)s->frame.p, s->stream));
    HIP_TRY(hipMemcpyAsync(out_sum, s->frame.p, out_bytes, hipMemcpyDeviceToHost, s->stream));
    return finish_render(s, cx, flags, stats);
}

// shared by prt_scatter_tiles / prt_scatter_frames: argument checks and the (cached) upload of the
// tile origins; then one scatter launch over n_tiles * tw * th slots
static int scatter_enqueue(void* scene, const float* d_packed, const int32_t* tile_ids, int n_tiles, int tw, int th,
                           int W, int H, int group_tiles, int64_t group_pitch, int n_frames, int64_t src_fpitch,
                           float* d_frame, int64_t dst_fpitch, void* stream) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    if (n_tiles < 0 || (n_tiles > 0 && (!tile_ids || !d_packed || !d_frame))) return fail(PRT_ERR_ARG, "NULL argument");
    if (tw < 1 || th < 1 || (tw & (tw - 1)) || (th & (th - 1)) || (int64_t)tw * th > (1 << 20))
        return fail(PRT_ERR_ARG, "tile width/height must be powers of two with tw*th <= 2^20");
    if (W < 1 || H < 1 || W > 65535 || H > 65535) return fail(PRT_ERR_ARG, "frame must be 1..65535 pixels per side");
    const int tiles_x = (W + tw - 1) / tw, tiles_y = (H + th - 1) / th;
    for (int i = 0; i < n_tiles; ++i)
        if (tile_ids[i] < -1 || tile_ids[i] >= tiles_x * tiles_y)
            return fail(PRT_ERR_ARG, "tile id out of range: " + std::to_string(tile_ids[i]));
    if ((int64_t)n_tiles * tw * th >= ((int64_t)1 << 31)) return fail(PRT_ERR_ARG, "too many slots in one call");
    if (n_tiles == 0) return PRT_OK;
    DeviceGuard g(s->device);
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    std::vector<uint32_t> xy = tile_origins(tile_ids, n_tiles, tiles_x, tw, th);
    // uploaded only when they differ from the last call's (a bench or an animation scatters the
    // same tile set every frame): a steady-state frame then neither copies nor waits on the host
    if (xy != s->scatter_xy_host) {
        // earlier scatters (on any stream) may still read the device copy, and the previous
        // upload its host copy: a changed tile set waits for the device once
        if (s->scatter_ev) HIP_TRY(hipDeviceSynchronize());
        else HIP_TRY(hipEventCreateWithFlags(&s->scatter_ev, hipEventDisableTiming));
        HIP_TRY(s->scatter_xy.ensure(sizeof(uint32_t) * (size_t)n_tiles));
        s->scatter_xy_host.swap(xy);
        HIP_TRY(hipMemcpyAsync(s->scatter_xy.p, s->scatter_xy_host.data(), sizeof(uint32_t) * (size_t)n_tiles,
                               hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(s->scatter_ev, st));
    } else if (hipEventQuery(s->scatter_ev) != hipSuccess) {
        // same tile set, uploaded on a stream that may not have reached the copy yet
        HIP_TRY(hipStreamWaitEvent(st, s->scatter_ev, 0));
    }
    const int log_tw = __builtin_ctz((unsigned)tw), log_tpx = __builtin_ctz((unsigned)(tw * th));
    HIP_TRY(launch_scatter_frames(d_packed, (const uint32_t*)s->scatter_xy.p, n_tiles * tw * th, group_tiles * tw * th,
                                  group_pitch, n_frames, src_fpitch, dst_fpitch, log_tw, log_tpx, 0, 0, W, H, d_frame,
                                  st));
    return PRT_OK;
}

int prt_scatter_tiles(void* scene, const float* d_packed, const int32_t* tile_ids, int n_tiles, int tw, int th,
                      int W, int H, float* d_frame, void* stream) {
    return scatter_enqueue(scene, d_packed, tile_ids, n_tiles, tw, th, W, H, std::max(n_tiles, 1), 0, 1, 0, d_frame, 0,
                           stream);
}

int prt_scatter_frames(void* scene, const float* d_packed, const int32_t* tile_ids, int n_groups, int group_tiles,
                       int64_t group_pitch, int tw, int th, int W, int H, int n_frames, int64_t src_frame_pitch,
                       float* d_frames, void* stream) {
    if (n_groups < 0 || group_tiles < 1 || n_frames < 1 || n_frames > 65535)
        return fail(PRT_ERR_ARG, "need n_groups >= 0, group_tiles >= 1 and 1 <= n_frames <= 65535");
    const int64_t slot_f = (int64_t)tw * th * 3;
    if (group_pitch < 0 || src_frame_pitch < 0 || (n_groups > 1 && group_pitch < group_tiles * slot_f) ||
        (n_frames > 1 && src_frame_pitch < group_tiles * slot_f))
        return fail(PRT_ERR_ARG, "group_pitch / src_frame_pitch must hold a group's tiles");
    // a group holds all n_frames frames of its tiles: frame f of group g must not reach into group g + 1
    // 
    if (n_groups > 1 && group_pitch < (int64_t)(n_frames - 1) * src_frame_pitch + group_tiles * slot_f)
        return fail(PRT_ERR_ARG, "group_pitch must hold n_frames frames of a group at src_frame_pitch");
    if ((int64_t)n_groups * group_tiles >= ((int64_t)1 << 31)) return fail(PRT_ERR_ARG, "too many tiles");
    return scatter_enqueue(scene, d_packed, tile_ids, n_groups * group_tiles, tw, th, W, H, group_tiles, group_pitch,
                           n_frames, src_frame_pitch, d_frames, 3 * (int64_t)W * H, stream);
}

}  // extern "C"

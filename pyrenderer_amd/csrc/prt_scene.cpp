// prt_scene.cpp — the library's identity calls, host BVH handles, and a scene's life: validate, build
// the BVH, pack, upload, query the device, read the environment knobs; plus the calls of the size-only
// launch decisions (prt_plan.h: LDS footprints, the trace-kernel variant) for a scene (prt_host.h).
#include <chrono>
#include <cstdlib>
#include <new>

#include "prt_host.h"

namespace prt {

thread_local std::string g_err;

namespace {

int upload(DevBuf& b, const void* host, size_t bytes, size_t* total) {
    HIP_TRY(b.ensure(std::max<size_t>(bytes, 16)));
    if (bytes) HIP_TRY(hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice));
    *total += b.bytes;
    return PRT_OK;
}

// The buffers free themselves (DevBuf); what needs an order: the scene's device current, and the
// device idle before the render contexts' buffers (streams of the caller may still run on them) go.
void destroy_scene(Scene* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    if (!s->ctx.empty()) (void)hipDeviceSynchronize();
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->refit.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->rebuild.ev)
        if (e) (void)hipEventDestroy(e);
    if (s->scatter_ev) (void)hipEventDestroy(s->scatter_ev);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// the scene's sizes alone (all that the LDS footprints and the variant choice depend on, prt_plan.h) with
// the tree of `width` children per node, and the pooled kernel's stack for it
LdsSizes sizes_of(const Scene* s, int width) {
    const bool w8 = width == 8;
    return LdsSizes{(int)(w8 ? s->n_node8_f4 : s->n_node4_f4), (int)s->n_tri_f4, (int)s->n_tri, s->n_mat, s->n_lt,
                    s->n_light, w8 ? s->need8 : s->need4, w8 ? 8 : 4};
}

}  // namespace

int variant_width(const Scene* s, int var) { return variant_takes_width(var) ? s->lds_width : 4; }
int variant_need(const Scene* s, int var) { return variant_width(s, var) == 8 ? s->need8 : s->need4; }
LdsSizes scene_sizes(const Scene* s, int var) { return sizes_of(s, variant_width(s, var)); }

bool lds_fits4(const Scene* s, int var) { return lds_fits(scene_sizes(s, var)); }

// the traversal stack entries of variant `var` (LDS part for the spill variants; the pool kernel's
// instantiation set, its LDS stack being the launch parameter P.lds_stack)
int variant_stack(const Scene* s, int var) {
    return variant_pool(var) ? 16 : variant_spills(var) ? s->spill_lds : variant_width(s, var) == 8 ? s->stack8 : s->stack4;
}

// the variant a launch takes: the one the flags name, else the scene's default (the reference estimator's
// from the sizes of the tree its LDS kernels traverse, the MIS estimator's from the BVH4's)
int launch_variant(const Scene* s, uint32_t flags) {
    const int var = (int)((flags >> PRT_FLAG_VARIANT_SHIFT) & 0xFFu);
    if (var) return var;
    if (flags & PRT_FLAG_MIS_NEE) return choose_variant(sizes_of(s, 4), s->need4, s->stack4, true);
    const bool w8 = s->lds_width == 8;
    return choose_variant(sizes_of(s, s->lds_width), w8 ? s->need8 : s->need4, w8 ? s->stack8 : s->stack4, false);
}

// blocks per CU of variant `var`'s persistent grid (>= 1), queried once per (variant, stats)
int variant_occ(Scene* s, int var, bool stats) {
    int& occ = s->occ[2 * var + (stats ? 1 : 0)];
    const int stack = variant_stack(s, var);
    if (occ == 0)
        occ = std::max(1, trace_blocks_per_cu(stack, var, stats, variant_width(s, var),
                                              trace_smem_bytes(stack, var, scene_sizes(s, var))));
    return occ;
}

// Scene part of a trace launch's parameters (everything but the work description).
void scene_params(Scene* s, TraceParams& P) {
    std::memset(&P, 0, sizeof(P));   // lds_stack is set per launch (trace_setup)
    P.n_node_f4 = (int)s->n_node4_f4; P.n_tri_f4 = (int)s->n_tri_f4; P.n_tri = (int)s->n_tri;
    P.n_mat = s->n_mat; P.n_lt = s->n_lt; P.n_light = s->n_light;
    P.nodes = (const float4*)s->nodes4.p; P.tris = (const float4*)s->tris.p;
    P.tri_nm = (const float4*)s->tri_nm.p; P.tri_frame = (const float4*)s->tri_frame.p;
    P.mats = (const float*)s->mats.p;
    P.light_v = (const float4*)s->light_v.p; P.light_off = (const int*)s->light_off.p;
    P.dl_r = s->direct_rgb[0]; P.dl_g = s->direct_rgb[1]; P.dl_b = s->direct_rgb[2];
    P.resume_min = s->resume_min; P.pool_resume_min = s->pool_resume_min;
    P.stats = (unsigned long long*)s->stats.p;
    P.guard_trips = s->guard_trips;
    P.n_sph = (int)s->n_sph; P.sph = (const float4*)s->sph.p; P.sph_mat = (const int*)s->sph_mat.p;
    P.plain = s->plain ? 1 : 0; P.shade_fast = s->shade_fast ? 1 : 0;
    P.frame_spp = 0xFFFFFFFFu;   // one frame: global sample = s0 + j0 + the chunk's sample
    P.lds_width = 4;             // the BVH4; trace_setup switches the LDS reference kernels to the scene's width
}

namespace {

// device half of prt_scene_create: uploads, device properties, environment knobs
int fill_scene(Scene* s, const SceneArgs& a, const BvhHost& bvh, const PackedScene& pk) {
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(PRT_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    size_t* total = &s->device_bytes;
    {
        Bvh4Host b4;
        collapse_bvh4(bvh, &b4);
        s->n_node4_f4 = (int64_t)b4.nodes.size() / 4;
        s->stack4 = b4.stack_need <= 32 ? stack_variant(b4.stack_need - 1) : 0;
        s->need4 = b4.stack_need;
        if (int rc = upload(s->nodes4, b4.nodes.data(), sizeof(float) * b4.nodes.size(), total)) return rc;
        if (!wide_levels(b4.nodes.data(), b4.n_nodes, 4, &s->refit.level4, &s->refit.off4))
            return fail(PRT_ERR_INTERNAL, "internal: BVH4 child not numbered above its parent");
        std::vector<float> q4;
        quantize_bvh4(b4, bvh.pad, &q4);
        s->n_node4q_f4 = (int64_t)q4.size() / 4;
        if (int rc = upload(s->nodes4q, q4.data(), sizeof(float) * q4.size(), total)) return rc;
    }
    s->n_lt = pk.n_lt;
    s->n_tri_f4 = (int64_t)bvh.tris.size() / 4;
    // LDS-resident scenes also get the eight-wide tree; the width rule (prt_plan.h lds_width) says which of
    // the two their LDS reference kernels traverse
    s->lds_width_knob = (int)env_int("PRT_LDS_WIDTH", 0, 8, 0);
    if (lds_fits(sizes_of(s, 4))) {
        Bvh8Host b8;
        collapse_bvh8(bvh, &b8);
        s->n_node8_f4 = (int64_t)b8.nodes.size() / 4;
        s->need8 = b8.stack_need;
        s->stack8 = b8.stack_need <= 32 ? stack_variant(b8.stack_need - 1) : 0;
        if (!wide_levels(b8.nodes.data(), b8.n_nodes, 8, &s->refit.level8, &s->refit.off8))
            return fail(PRT_ERR_INTERNAL, "internal: BVH8 child not numbered above its parent");
        if (int rc = upload(s->nodes8, b8.nodes.data(), sizeof(float) * b8.nodes.size(), total)) return rc;
        s->lds_width = lds_width(sizes_of(s, 8), s->need8, s->lds_width_knob);
    }
    // what an update re-packs with and refits along (prt_host.h RefitState), host copies only
    s->refit.order = bvh.order;
    s->refit.tri_mat.assign(a.tri_mat, a.tri_mat + a.n_tri);
    s->refit.sph_mat.assign(a.sph_mat, a.sph_mat + a.n_sph);
    s->refit.mat.assign(a.mat, a.mat + 8 * (size_t)a.n_mat);
    s->refit.light_off.assign(a.light_off, a.light_off + a.n_light + 1);
    s->refit.light_tri.assign(a.light_tri, a.light_tri + a.light_off[a.n_light]);
    s->n_sph = a.n_sph;
    s->plain = pk.plain;
    s->shade_fast = pk.shade_fast;
    if (int rc = upload(s->tris, bvh.tris.data(), sizeof(float) * bvh.tris.size(), total)) return rc;
    if (int rc = upload(s->tri_nm, pk.tri_nm.data(), sizeof(float) * pk.tri_nm.size(), total)) return rc;
    if (int rc = upload(s->tri_frame, pk.tri_frame.data(), sizeof(float) * pk.tri_frame.size(), total)) return rc;
    if (int rc = upload(s->mats, a.mat, sizeof(float) * 8 * (size_t)a.n_mat, total)) return rc;
    if (int rc = upload(s->light_v, pk.light_v.data(), sizeof(float) * pk.light_v.size(), total)) return rc;
    if (int rc = upload(s->light_off, a.light_off, sizeof(int32_t) * (size_t)(a.n_light + 1), total)) return rc;
    if (int rc = upload(s->sph, a.sph, sizeof(float) * 4 * (size_t)a.n_sph, total)) return rc;
    if (int rc = upload(s->sph_mat, a.sph_mat, sizeof(int32_t) * (size_t)a.n_sph, total)) return rc;
    if ((e = s->work.ensure(64)) != hipSuccess || (e = s->stats.ensure(8 * kStatWords)) != hipSuccess)
        return fail(PRT_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    // the hit-query watchdog flag is read by prt_check_faults before any hit query ran
    if ((e = hipMemset(s->work.p, 0, 64)) != hipSuccess) return fail(PRT_ERR_HIP, hipGetErrorString(e));
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, s->device)) != hipSuccess) return fail(PRT_ERR_HIP, hipGetErrorString(e));
    s->cus = prop.multiProcessorCount;
    s->leaf_exit = (int)env_int("PRT_LEAF_EXIT", 0, 64, s->leaf_exit);
    s->leaf_break = (int)env_int("PRT_LEAF_BREAK", 0, 64, s->leaf_break);
    if (const char* wc = std::getenv("PRT_WAVE_CLOCK")) s->wave_clock_path = wc;
    s->guard_trips = (uint32_t)env_int("PRT_GUARD_TRIPS", 1, UINT32_MAX, s->guard_trips);
    s->resume_min = (int)env_int("PRT_RESUME_MIN", 1, 64, s->resume_min);
    s->pool_resume_min = (int)env_int("PRT_POOL_RESUME_MIN", 0, 64, s->pool_resume_min);
    s->spill_lds = spill_lds_entries(env_int("PRT_SPILL_LDS", INT32_MIN, INT32_MAX, s->spill_lds));
    s->blocks_per_cu = variant_occ(s, launch_variant(s, 0), false);
    if (const long long cb = env_int("PRT_CHUNK_BYTES", 1LL << 20, INT64_MAX, 0)) {
        s->chunk_bytes = (size_t)cb;
    } else {
        // the default budget takes at most a quarter of the memory free at scene creation (16 GiB
        // of an idle MI355X's 288 GB); enqueue_render also caps it by the memory free when a
        // render stream's buffers grow
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
            s->chunk_bytes = std::max<size_t>((size_t)1 << 28, std::min(s->chunk_bytes, free_b / 4));
    }
    return PRT_OK;
}

// first update: the device copies of the tree's order and level lists, the slot bounds and the
// original-order vertices
int refit_resident(Scene* s) {
    RefitState& r = s->refit;
    if (r.resident) return PRT_OK;
    size_t* total = &s->device_bytes;
    if (int rc = upload(r.d_order, r.order.data(), sizeof(int32_t) * r.order.size(), total)) return rc;
    if (int rc = upload(r.d_level4, r.level4.data(), sizeof(int32_t) * r.level4.size(), total)) return rc;
    if (int rc = upload(r.d_level8, r.level8.data(), sizeof(int32_t) * r.level8.size(), total)) return rc;
    HIP_TRY(r.d_bounds.ensure(std::max<size_t>(sizeof(float) * 6 * r.order.size(), 16)));
    HIP_TRY(r.d_tri_v.ensure(std::max<size_t>(sizeof(float) * 9 * (size_t)s->n_tri, 16)));
    *total += r.d_bounds.bytes + r.d_tri_v.bytes;
    for (hipEvent_t& e : r.ev) HIP_TRY(hipEventCreate(&e));
    r.resident = true;
    return PRT_OK;
}

int put(DevBuf& b, const void* host, size_t bytes, hipStream_t stream) {
    if (bytes > b.bytes) return fail(PRT_ERR_INTERNAL, "internal: update larger than the scene's buffer");
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, stream));
    return PRT_OK;
}

// one tree's levels, deepest first, one launch each
int refit_tree(int width, DevBuf& nodes, const DevBuf& level, const std::vector<int64_t>& off, const DevBuf& bounds,
               float pad, hipStream_t stream) {
    for (size_t l = off.size() - 1; l-- > 0;)
        HIP_TRY(launch_refit_level(width, (float*)nodes.p, (const int32_t*)level.p + off[l], off[l + 1] - off[l],
                                   (const float*)bounds.p, pad, stream));
    return PRT_OK;
}

// device half of prt_scene_update (validated arguments, packed shading data)
int update_scene(Scene* s, const float* tri_v, const float* sph, const PackedScene& pk, float pad) {
    RefitState& r = s->refit;
    // no render of this scene may be in flight on any of its streams while its buffers change
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = refit_resident(s)) return rc;
    hipStream_t st = s->stream;
    HIP_TRY(hipEventRecord(r.ev[0], st));
    if (int rc = put(r.d_tri_v, tri_v, sizeof(float) * 9 * (size_t)s->n_tri, st)) return rc;
    if (int rc = put(s->tri_nm, pk.tri_nm.data(), sizeof(float) * pk.tri_nm.size(), st)) return rc;
    if (int rc = put(s->tri_frame, pk.tri_frame.data(), sizeof(float) * pk.tri_frame.size(), st)) return rc;
    if (int rc = put(s->light_v, pk.light_v.data(), sizeof(float) * pk.light_v.size(), st)) return rc;
    if (int rc = put(s->sph, sph, sizeof(float) * 4 * (size_t)s->n_sph, st)) return rc;
    HIP_TRY(hipEventRecord(r.ev[1], st));
    HIP_TRY(launch_refit_tris((const float*)r.d_tri_v.p, (const int32_t*)r.d_order.p, (int64_t)r.order.size(),
                              (float4*)s->tris.p, (float*)r.d_bounds.p, st));
    HIP_TRY(hipEventRecord(r.ev[2], st));
    if (int rc = refit_tree(4, s->nodes4, r.d_level4, r.off4, r.d_bounds, pad, st)) return rc;
    if (s->n_node8_f4 > 0)
        if (int rc = refit_tree(8, s->nodes8, r.d_level8, r.off8, r.d_bounds, pad, st)) return rc;
    HIP_TRY(hipEventRecord(r.ev[3], st));
    HIP_TRY(launch_refit_quantize((const float*)s->nodes4.p, s->n_node4_f4 / kNode4F4, pad, (float*)s->nodes4q.p, st));
    HIP_TRY(hipEventRecord(r.ev[4], st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 4; ++k) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r.ev[k], r.ev[k + 1]));
        r.ms[k + 1] = ms;
    }
    s->shade_fast = pk.shade_fast;
    s->blocks_per_cu = variant_occ(s, launch_variant(s, 0), false);
    return PRT_OK;
}

// a buffer that grows only when it holds less than `bytes`; the scene's device bytes follow it
int grow(DevBuf& b, size_t bytes, size_t* total) {
    const size_t had = b.bytes;
    const hipError_t e = b.ensure(std::max<size_t>(bytes, 16));
    *total = *total - had + b.bytes;
    if (e != hipSuccess) return fail(PRT_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return PRT_OK;
}

// Stage 4 of a rebuild for one width: the levels top-down (one count read back per level), then the node
// records into `nodes`, grown to the tree's size first.  The keys' binary tree is in b.split.
int build_wide(Scene* s, int width, DevBuf& nodes, LbvhLevels* lv, int* need) {
    RebuildState& b = s->rebuild;
    hipStream_t st = s->stream;
    const int64_t n = s->n_tri, cap = lbvh_node_capacity(n), widest = n / 2 + 1;
    auto* items = (LbvhItem*)b.items.p;
    HIP_TRY(launch_lbvh_root(items, n, (int32_t*)b.max_anc.p, st));
    *lv = LbvhLevels();
    lv->push(1, cap, widest);
    for (;;) {
        const int64_t base = lv->off[(size_t)lv->depth()], count = lv->n_nodes() - base;
        HIP_TRY(launch_lbvh_level(width, items, base, count, lv->n_nodes(), (const int32_t*)b.split.p, s->max_leaf,
                                  (int32_t*)b.cnt.p, (int32_t*)b.off.p, (int32_t*)b.child0.p, (int32_t*)b.max_anc.p,
                                  b.temp.p, b.temp.bytes, st));
        int32_t next = 0;
        HIP_TRY(hipMemcpyAsync(&next, (const int32_t*)b.off.p + count, sizeof next, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (next == 0) break;
        if (!lv->push(next, cap, widest)) return fail(PRT_ERR_INTERNAL, "internal: rebuilt tree outgrew its bound");
    }
    int32_t max_anc = 0;
    HIP_TRY(hipMemcpyAsync(&max_anc, b.max_anc.p, sizeof max_anc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *need = wide_stack_need(max_anc, width);
    const size_t node_bytes = sizeof(float) * 4 * (size_t)(width == 8 ? kNode8F4 : kNode4F4);
    if (int rc = grow(nodes, node_bytes * (size_t)lv->n_nodes(), &s->device_bytes)) return rc;
    HIP_TRY(launch_lbvh_emit(width, items, (const int32_t*)b.child0.p, lv->n_nodes(), (const int32_t*)b.split.p,
                             s->max_leaf, (float*)nodes.p, st));
    return PRT_OK;
}

// device half of prt_scene_rebuild (validated arguments, packed shading data): DESIGN.md §14
int rebuild_scene(Scene* s, const float* tri_v, const float* sph, const PackedScene& pk, float pad) {
    RefitState& r = s->refit;
    RebuildState& b = s->rebuild;
    const int64_t n = s->n_tri;
    // no render of this scene may be in flight on any of its streams while its buffers change
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = refit_resident(s)) return rc;
    size_t* total = &s->device_bytes;
    const LbvhScratch z = lbvh_scratch(n);
    size_t temp_bytes = 0;
    HIP_TRY(lbvh_temp_bytes(n, &temp_bytes));
    DevBuf* words[] = {&b.codes, &b.ids, &b.codes_sorted, &b.split, &b.child0};
    for (DevBuf* w : words)
        if (int rc = grow(*w, z.word, total)) return rc;
    if (int rc = grow(b.cen, z.cen, total)) return rc;
    if (int rc = grow(b.cbox, 32, total)) return rc;
    if (int rc = grow(b.keys, z.key, total)) return rc;
    if (int rc = grow(b.items, z.item, total)) return rc;
    if (int rc = grow(b.cnt, z.count, total)) return rc;
    if (int rc = grow(b.off, z.count, total)) return rc;
    if (int rc = grow(b.max_anc, 16, total)) return rc;
    if (int rc = grow(b.temp, temp_bytes, total)) return rc;
    for (hipEvent_t& e : b.ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    hipStream_t st = s->stream;
    HIP_TRY(hipEventRecord(b.ev[0], st));
    if (int rc = put(r.d_tri_v, tri_v, sizeof(float) * 9 * (size_t)n, st)) return rc;
    if (int rc = put(s->tri_nm, pk.tri_nm.data(), sizeof(float) * pk.tri_nm.size(), st)) return rc;
    if (int rc = put(s->tri_frame, pk.tri_frame.data(), sizeof(float) * pk.tri_frame.size(), st)) return rc;
    if (int rc = put(s->light_v, pk.light_v.data(), sizeof(float) * pk.light_v.size(), st)) return rc;
    if (int rc = put(s->sph, sph, sizeof(float) * 4 * (size_t)s->n_sph, st)) return rc;
    HIP_TRY(hipEventRecord(b.ev[1], st));
    HIP_TRY(launch_lbvh_codes((const float*)r.d_tri_v.p, n, (float*)b.cen.p, (float*)b.cbox.p, (uint32_t*)b.codes.p,
                              (uint32_t*)b.ids.p, b.temp.p, b.temp.bytes, st));
    HIP_TRY(hipEventRecord(b.ev[2], st));
    // one slot per triangle: the order's buffer, sized for creation's slots, holds them
    HIP_TRY(launch_lbvh_sort((const uint32_t*)b.codes.p, (const uint32_t*)b.ids.p, n, (uint32_t*)b.codes_sorted.p,
                             (int32_t*)r.d_order.p, (uint64_t*)b.keys.p, b.temp.p, b.temp.bytes, st));
    HIP_TRY(hipEventRecord(b.ev[3], st));
    HIP_TRY(launch_lbvh_topology((const uint64_t*)b.keys.p, n, (int32_t*)b.split.p, st));
    HIP_TRY(hipEventRecord(b.ev[4], st));
    LbvhLevels lv4, lv8;
    int need4 = 0, need8 = 0;
    if (int rc = build_wide(s, 4, s->nodes4, &lv4, &need4)) return rc;
    s->n_tri_f4 = kTriF4 * n;
    s->n_node4_f4 = lv4.n_nodes() * kNode4F4;
    s->n_node4q_f4 = lv4.n_nodes() * kNodeQF4;
    s->need4 = need4;
    s->stack4 = need4 <= 32 ? stack_variant(need4 - 1) : 0;
    s->n_nodes = lv4.n_nodes();
    s->depth = lv4.depth();
    s->n_node8_f4 = 0;
    s->need8 = s->stack8 = 0;
    s->lds_width = 4;
    // LDS-resident scenes also get the eight-wide tree, and the width rule again (fill_scene)
    if (lds_fits(sizes_of(s, 4))) {
        if (int rc = build_wide(s, 8, s->nodes8, &lv8, &need8)) return rc;
        s->n_node8_f4 = lv8.n_nodes() * kNode8F4;
        s->need8 = need8;
        s->stack8 = need8 <= 32 ? stack_variant(need8 - 1) : 0;
        s->lds_width = lds_width(sizes_of(s, 8), s->need8, s->lds_width_knob);
    }
    if (int rc = grow(s->nodes4q, sizeof(float) * 4 * (size_t)s->n_node4q_f4, total)) return rc;
    if (int rc = grow(r.d_level4, sizeof(int32_t) * (size_t)lv4.n_nodes(), total)) return rc;
    if (int rc = grow(r.d_level8, sizeof(int32_t) * (size_t)lv8.n_nodes(), total)) return rc;
    HIP_TRY(launch_lbvh_iota((int32_t*)r.d_level4.p, lv4.n_nodes(), st));
    HIP_TRY(launch_lbvh_iota((int32_t*)r.d_level8.p, lv8.n_nodes(), st));
    HIP_TRY(hipEventRecord(b.ev[5], st));
    // stage 5: the refit's own launches on the new order and level lists
    r.off4 = lv4.off;
    r.off8 = lv8.off;
    r.level4 = iota_list(lv4.n_nodes());
    r.level8 = iota_list(lv8.n_nodes());
    HIP_TRY(launch_refit_tris((const float*)r.d_tri_v.p, (const int32_t*)r.d_order.p, n, (float4*)s->tris.p,
                              (float*)r.d_bounds.p, st));
    if (int rc = refit_tree(4, s->nodes4, r.d_level4, r.off4, r.d_bounds, pad, st)) return rc;
    if (s->n_node8_f4 > 0)
        if (int rc = refit_tree(8, s->nodes8, r.d_level8, r.off8, r.d_bounds, pad, st)) return rc;
    HIP_TRY(hipEventRecord(b.ev[6], st));
    HIP_TRY(launch_refit_quantize((const float*)s->nodes4.p, lv4.n_nodes(), pad, (float*)s->nodes4q.p, st));
    HIP_TRY(hipEventRecord(b.ev[7], st));
    r.order.resize((size_t)n);
    if (n) HIP_TRY(hipMemcpyAsync(r.order.data(), r.d_order.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int k = 0; k < 7; ++k) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, b.ev[k], b.ev[k + 1]));
        b.ms[k + 1] = ms;
    }
    const int64_t info[8] = {lv4.n_nodes(), lv4.depth(), need4, s->n_node8_f4 ? lv8.n_nodes() : 0,
                             s->n_node8_f4 ? lv8.depth() : 0, need8, s->lds_width, n};
    std::memcpy(b.info, info, sizeof info);
    ++b.count;
    s->shade_fast = pk.shade_fast;
    std::memset(s->occ, 0, sizeof s->occ);   // the blocks per CU were those of the old tree's stacks
    s->blocks_per_cu = variant_occ(s, launch_variant(s, 0), false);
    return PRT_OK;
}

}  // namespace
}  // namespace prt

using namespace prt;

extern "C" {

int prt_abi_version(void) { return PRT_ABI_VERSION; }

const char* prt_last_error(void) { return g_err.c_str(); }

int prt_device_count(int* n) {
    if (!n) return fail(PRT_ERR_ARG, "n is NULL");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return PRT_OK;
}

int prt_bvh_build(const float* tri_v, int64_t n_tri, int32_t max_leaf, void** out_bvh) {
    if (!out_bvh || (n_tri > 0 && !tri_v)) return fail(PRT_ERR_ARG, "NULL argument");
    auto* b = new (std::nothrow) BvhHost();
    if (!b) return fail(PRT_ERR_OOM, "host allocation failed");
    std::string err;
    try {
        if (!build_bvh(tri_v, n_tri, max_leaf, b, &err)) { delete b; return fail(PRT_ERR_ARG, err); }
    } catch (const std::bad_alloc&) {
        delete b;
        return fail(PRT_ERR_OOM, "host allocation failed during BVH build");
    }
    *out_bvh = b;
    return PRT_OK;
}

int prt_bvh_info(void* bvh, int64_t* info6) {
    auto* b = (BvhHost*)bvh;
    if (!b || !info6) return fail(PRT_ERR_ARG, "NULL argument");
    int32_t padbits;
    std::memcpy(&padbits, &b->pad, 4);
    info6[0] = b->n_nodes; info6[1] = b->depth; info6[2] = b->n_leaves; info6[3] = (int64_t)b->order.size();
    info6[4] = padbits; info6[5] = (int64_t)(b->sah_cost * 1000.0 + 0.5);
    return PRT_OK;
}

int prt_bvh_export(void* bvh, float* nodes, float* tris, int32_t* order) {
    auto* b = (BvhHost*)bvh;
    if (!b) return fail(PRT_ERR_ARG, "NULL argument");
    if (nodes) std::memcpy(nodes, b->nodes.data(), sizeof(float) * b->nodes.size());
    if (tris) std::memcpy(tris, b->tris.data(), sizeof(float) * b->tris.size());
    if (order) std::memcpy(order, b->order.data(), sizeof(int32_t) * b->order.size());
    return PRT_OK;
}

int prt_bvh_collapse(void* bvh, int32_t width, int64_t* info4, float* nodes) {
    auto* b = (BvhHost*)bvh;
    if (!b || !info4) return fail(PRT_ERR_ARG, "NULL argument");
    if (width != 4 && width != 8) return fail(PRT_ERR_ARG, "width must be 4 or 8");
    try {
        Bvh4Host b4;
        Bvh8Host b8;
        if (width == 4) collapse_bvh4(*b, &b4);
        else collapse_bvh8(*b, &b8);
        const std::vector<float>& f = width == 4 ? b4.nodes : b8.nodes;
        info4[0] = width == 4 ? b4.n_nodes : b8.n_nodes;
        info4[1] = width == 4 ? b4.depth : b8.depth;
        info4[2] = width == 4 ? b4.stack_need : b8.stack_need;
        info4[3] = 4 * (width == 4 ? kNode4F4 : kNode8F4);
        if (nodes) std::memcpy(nodes, f.data(), sizeof(float) * f.size());
    } catch (const std::bad_alloc&) {
        return fail(PRT_ERR_OOM, "host allocation failed during the collapse");
    }
    return PRT_OK;
}

void prt_bvh_destroy(void* bvh) { delete (BvhHost*)bvh; }

int prt_scene_create(int device, const float* tri_v, const float* tri_n, const int32_t* tri_mat, int64_t n_tri,
                     const float* sph, const int32_t* sph_mat, int64_t n_sph, const float* mat, int32_t n_mat,
                     const int32_t* light_tri, const int32_t* light_off, int32_t n_light, const float* direct_rgb,
                     void** out_scene) {
    if (!out_scene) return fail(PRT_ERR_ARG, "out_scene is NULL");
    *out_scene = nullptr;
    const SceneArgs a{tri_v, tri_n, tri_mat, n_tri, sph, sph_mat, n_sph, mat, n_mat, light_tri, light_off, n_light};
    std::string err;
    if (!validate_scene(a, &err)) return fail(PRT_ERR_ARG, err);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PRT_ERR_HIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(PRT_ERR_ARG, "device index out of range");

    BvhHost bvh;
    PackedScene pk;
    const int max_leaf = (int)env_int("PRT_MAX_LEAF", INT32_MIN, INT32_MAX, 4);
    try {
        if (!build_bvh(tri_v, n_tri, max_leaf, &bvh, &err))
            return fail(PRT_ERR_ARG, err);
        pack_scene(a, &pk);
    } catch (const std::bad_alloc&) {
        return fail(PRT_ERR_OOM, "host allocation failed during BVH build");
    }
    auto* s = new (std::nothrow) Scene();
    if (!s) return fail(PRT_ERR_OOM, "host allocation failed");
    s->device = device;
    s->max_leaf = max_leaf;
    s->n_tri = n_tri;
    s->n_nodes = bvh.n_nodes;
    s->depth = bvh.depth;
    s->n_light = n_light;
    s->n_mat = n_mat;
    if (direct_rgb) std::memcpy(s->direct_rgb, direct_rgb, sizeof(float) * 3);
    DeviceGuard g(device);
    if (int rc = fill_scene(s, a, bvh, pk)) { destroy_scene(s); return rc; }
    *out_scene = s;
    return PRT_OK;
}

int prt_scene_info(void* scene, int64_t* info8) {
    auto* s = (Scene*)scene;
    if (!s || !info8) return fail(PRT_ERR_ARG, "NULL argument");
    info8[0] = s->device; info8[1] = s->n_tri; info8[2] = s->n_nodes; info8[3] = s->depth;
    info8[4] = s->stack4; info8[5] = (int64_t)s->device_bytes; info8[6] = s->blocks_per_cu; info8[7] = s->cus;
    return PRT_OK;
}

void prt_scene_destroy(void* scene) { destroy_scene((Scene*)scene); }

int prt_scene_update(void* scene, const float* tri_v, const float* tri_n, const float* sph) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    if (!validate_update(tri_v, tri_n, s->n_tri, sph, s->n_sph, &err)) return fail(PRT_ERR_ARG, err);
    RefitState& r = s->refit;
    const SceneArgs a{tri_v, tri_n, r.tri_mat.data(), s->n_tri, sph, r.sph_mat.data(), s->n_sph, r.mat.data(), s->n_mat,
                      r.light_tri.data(), r.light_off.data(), s->n_light};
    PackedScene pk;
    float pad = 0.0f;
    try {
        pack_scene(a, &pk);
        pad = bvh_pad(tri_v, s->n_tri);
    } catch (const std::bad_alloc&) {
        return fail(PRT_ERR_OOM, "host allocation failed during the scene update");
    }
    r.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    DeviceGuard g(s->device);
    return update_scene(s, tri_v, sph, pk, pad);
}

int prt_scene_rebuild(void* scene, const float* tri_v, const float* tri_n, const float* sph) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    const auto t0 = std::chrono::steady_clock::now();
    std::string err;
    if (!validate_update(tri_v, tri_n, s->n_tri, sph, s->n_sph, &err)) return fail(PRT_ERR_ARG, err);
    if (s->n_tri >= kLbvhMaxSlots) return fail(PRT_ERR_ARG, "a rebuild takes fewer than 2^28 triangles");
    RefitState& r = s->refit;
    const SceneArgs a{tri_v, tri_n, r.tri_mat.data(), s->n_tri, sph, r.sph_mat.data(), s->n_sph, r.mat.data(), s->n_mat,
                      r.light_tri.data(), r.light_off.data(), s->n_light};
    PackedScene pk;
    float pad = 0.0f;
    try {
        pack_scene(a, &pk);
        pad = bvh_pad(tri_v, s->n_tri);
    } catch (const std::bad_alloc&) {
        return fail(PRT_ERR_OOM, "host allocation failed during the scene rebuild");
    }
    s->rebuild.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    DeviceGuard g(s->device);
    try {
        return rebuild_scene(s, tri_v, sph, pk, pad);
    } catch (const std::bad_alloc&) {
        return fail(PRT_ERR_OOM, "host allocation failed during the scene rebuild");
    }
}

int prt_scene_rebuild_info(void* scene, int64_t* info8, double* ms8) {
    auto* s = (Scene*)scene;
    if (!s) return fail(PRT_ERR_ARG, "scene is NULL");
    if (s->rebuild.count == 0) return fail(PRT_ERR_ARG, "the scene has not been rebuilt");
    if (info8) std::memcpy(info8, s->rebuild.info, sizeof s->rebuild.info);
    if (ms8) std::memcpy(ms8, s->rebuild.ms, sizeof s->rebuild.ms);
    return PRT_OK;
}

int prt_scene_download(void* scene, int which, void* out, int64_t bytes) {
    auto* s = (Scene*)scene;
    if (!s || !out) return fail(PRT_ERR_ARG, "NULL argument");
    const bool ask = (which & PRT_BUF_BYTES) != 0;
    const DevBuf* b = nullptr;
    int64_t have = 0;
    switch (which & ~PRT_BUF_BYTES) {
        case PRT_BUF_NODES4: b = &s->nodes4; have = 16 * s->n_node4_f4; break;
        case PRT_BUF_NODES4Q: b = &s->nodes4q; have = 16 * s->n_node4q_f4; break;
        case PRT_BUF_NODES8: b = &s->nodes8; have = 16 * s->n_node8_f4; break;
        case PRT_BUF_TRIS: b = &s->tris; have = 16 * s->n_tri_f4; break;
        case PRT_BUF_TRI_NM: b = &s->tri_nm; have = 16 * std::max<int64_t>(s->n_tri, 1); break;
        case PRT_BUF_TRI_FRAME: b = &s->tri_frame; have = 96 * std::max<int64_t>(s->n_tri, 1); break;
        case PRT_BUF_LIGHT_V: b = &s->light_v; have = 64 * (int64_t)s->n_lt; break;
        case PRT_BUF_SPH: b = &s->sph; have = 16 * s->n_sph; break;
        case PRT_BUF_UPDATE_MS: have = (int64_t)sizeof(s->refit.ms); break;
        default: return fail(PRT_ERR_ARG, "unknown buffer");
    }
    if (ask) {
        if (bytes != (int64_t)sizeof(int64_t)) return fail(PRT_ERR_ARG, "a size query writes one int64");
        std::memcpy(out, &have, sizeof(int64_t));
        return PRT_OK;
    }
    if (bytes != have) return fail(PRT_ERR_ARG, "buffer holds " + std::to_string(have) + " bytes, not " + std::to_string(bytes));
    if (!b) {
        std::memcpy(out, s->refit.ms, sizeof(s->refit.ms));
        return PRT_OK;
    }
    if ((size_t)have > b->bytes) return fail(PRT_ERR_INTERNAL, "internal: buffer shorter than its contents");
    DeviceGuard g(s->device);
    HIP_TRY(hipDeviceSynchronize());
    if (have) HIP_TRY(hipMemcpy(out, b->p, (size_t)have, hipMemcpyDeviceToHost));
    return PRT_OK;
}

int prt_scene_kernel(void* scene, int32_t* out4) { return prt_launch_kernel(scene, INT64_MAX, 0, out4); }

int prt_launch_kernel(void* scene, int64_t n_items, uint32_t flags, int32_t* out4) {
    auto* s = (Scene*)scene;
    if (!s || !out4) return fail(PRT_ERR_ARG, "NULL argument");
    if (n_items < 0) return fail(PRT_ERR_ARG, "n_items < 0");
    int var = launch_variant(s, flags);
    out4[0] = var;
    out4[1] = variant_width(s, var);
    out4[2] = (variant_uses_lds(var) ? 1 : 0) | (variant_quantized(var) ? 2 : 0) | (s->shade_fast ? 4 : 0) |
              (s->plain ? 8 : 0);
    // the pooled kernel's LDS stack is sized to its tree's exact bound (P.lds_stack)
    out4[3] = variant_pool(var) ? variant_need(s, var) : variant_stack(s, var);
    return PRT_OK;
}

}  // extern "C"

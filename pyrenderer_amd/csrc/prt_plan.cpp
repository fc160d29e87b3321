// prt_plan.cpp — see prt_plan.h.  Compiled with the library's flags (-ffp-contract=off): tri_frame and
// the camera terms feed bit-exact shading, so their f32 operation order is part of the contract.
#include "prt_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace prt {
namespace {

float bits_f(int32_t v) { float f; std::memcpy(&f, &v, 4); return f; }

// rotate_to / rotate_z_to rows (mathematics/mat4_taichi.py:9-52) for a normal, in the kernel's f32
// arithmetic: rows (x, z, v) with v = normalize(n), x = normalize(v x (0,1,0)), z = normalize(x x v).
struct F3 { float x, y, z; };
F3 f3_norm(F3 a) {
    float l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return F3{a.x / l, a.y / l, a.z / l};
}
F3 f3_cross(F3 a, F3 b) { return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
void frame_rows(F3 n, float* out12) {
    F3 v = f3_norm(n);
    F3 r1, r2, r3;
    if (v.y == 1.0f) {
        r1 = F3{1, 0, 0}; r2 = F3{0, 0, 1}; r3 = F3{0, 1, 0};
    } else if (v.y == -1.0f) {
        r1 = F3{1, 0, 0}; r2 = F3{0, 0, 1}; r3 = F3{0, -1, 0};
    } else {
        F3 x = f3_norm(f3_cross(v, F3{0.0f, 1.0f, 0.0f}));
        F3 z = f3_norm(f3_cross(x, v));
        r1 = x; r2 = z; r3 = v;
    }
    const F3 rows[3] = {r1, r2, r3};
    for (int k = 0; k < 3; ++k) {
        out12[4 * k] = rows[k].x; out12[4 * k + 1] = rows[k].y; out12[4 * k + 2] = rows[k].z; out12[4 * k + 3] = 0.0f;
    }
}

bool bad(std::string* err, const std::string& msg) { *err = msg; return false; }

}  // namespace

bool validate_scene(const SceneArgs& a, std::string* err) {
    if (a.n_tri < 0 || (a.n_tri > 0 && (!a.tri_v || !a.tri_n || !a.tri_mat))) return bad(err, "bad triangle arrays");
    if (a.n_sph < 0 || (a.n_sph > 0 && (!a.sph || !a.sph_mat))) return bad(err, "bad sphere arrays");
    for (int64_t k = 0; k < a.n_sph; ++k) {
        if (a.sph_mat[k] < 0 || a.sph_mat[k] >= a.n_mat) return bad(err, "sphere material id out of range");
        if (!(a.sph[4 * k + 3] > 0.0f)) return bad(err, "sphere radius must be > 0");
    }
    if (a.n_tri + a.n_sph >= ((int64_t)1 << 31)) return bad(err, "too many primitives");
    if (a.n_mat < 1 || !a.mat) return bad(err, "need at least one material");
    if (a.n_light < 1 || !a.light_off || !a.light_tri) return bad(err, "There is no lights!!! (n_light < 1)");
    for (int64_t i = 0; i < a.n_tri; ++i)
        if (a.tri_mat[i] < 0 || a.tri_mat[i] >= a.n_mat)
            return bad(err, "material id out of range at triangle " + std::to_string(i));
    if (a.light_off[0] != 0) return bad(err, "light_off[0] must be 0");
    for (int l = 0; l < a.n_light; ++l)
        if (a.light_off[l + 1] <= a.light_off[l]) return bad(err, "every light needs >= 1 triangle");
    for (int32_t k = 0; k < a.light_off[a.n_light]; ++k)
        if (a.light_tri[k] < 0 || a.light_tri[k] >= a.n_tri) return bad(err, "light triangle out of range");
    return true;
}

void pack_scene(const SceneArgs& a, PackedScene* out) {
    const int64_t n_tri = a.n_tri;
    out->tri_nm.assign((size_t)std::max<int64_t>(n_tri, 1) * 4, 0.0f);
    out->tri_frame.assign((size_t)std::max<int64_t>(n_tri, 1) * 24, 0.0f);
    for (int64_t i = 0; i < n_tri; ++i) {
        const F3 nn{a.tri_n[3 * i], a.tri_n[3 * i + 1], a.tri_n[3 * i + 2]};
        float* nm = out->tri_nm.data() + 4 * i;
        nm[0] = nn.x; nm[1] = nn.y; nm[2] = nn.z;
        nm[3] = bits_f(a.tri_mat[i]);
        frame_rows(nn, out->tri_frame.data() + 24 * i);
        frame_rows(F3{-nn.x, -nn.y, -nn.z}, out->tri_frame.data() + 24 * i + 12);
    }
    out->n_lt = a.light_off[a.n_light];
    out->light_v.assign((size_t)out->n_lt * 16, 0.0f);
    for (int k = 0; k < out->n_lt; ++k) {
        const int64_t t = a.light_tri[k];
        float* lv = out->light_v.data() + 16 * (size_t)k;
        for (int c = 0; c < 3; ++c) {
            lv[c] = a.tri_v[9 * t + c];
            lv[4 + c] = a.tri_v[9 * t + 3 + c];
            lv[8 + c] = a.tri_v[9 * t + 6 + c];
            lv[12 + c] = a.tri_n[3 * t + c];
        }
        lv[15] = bits_f(a.tri_mat[t]);
    }
    out->plain = a.n_sph == 0;
    for (int32_t i = 0; i < a.n_mat; ++i)
        if (a.mat[8 * i + 5] == 2.0f || a.mat[8 * i + 5] == 3.0f) out->plain = false;   // metal / dielectric
    // the shading quotients' cheap guards (prt_math.h lambert_div / nee_div) assume albedos and
    // emitters in [2^-40, 2^40] and face normals of length in [0.5, 2]; other scenes keep div3's guard
    out->shade_fast = true;
    for (int32_t i = 0; i < a.n_mat && out->shade_fast; ++i)
        for (int c = 0; c < 3; ++c) {
            const float r = a.mat[8 * i + c];
            if (!(r >= 0x1p-40f && r <= 0x1p40f)) out->shade_fast = false;
        }
    for (int64_t i = 0; i < n_tri && out->shade_fast; ++i) {
        const double x = a.tri_n[3 * i], y = a.tri_n[3 * i + 1], z = a.tri_n[3 * i + 2];
        const double l2 = x * x + y * y + z * z;
        if (!(l2 >= 0.25 && l2 <= 4.0)) out->shade_fast = false;
    }
}

bool validate_update(const float* tri_v, const float* tri_n, int64_t n_tri, const float* sph, int64_t n_sph,
                     std::string* err) {
    if (n_tri > 0 && (!tri_v || !tri_n)) return bad(err, "bad triangle arrays");
    if (n_sph > 0 && !sph) return bad(err, "bad sphere array");
    for (int64_t i = 0; i < 9 * n_tri; ++i)
        if (!std::isfinite(tri_v[i])) return bad(err, "non-finite vertex in triangle " + std::to_string(i / 9));
    for (int64_t i = 0; i < 3 * n_tri; ++i)
        if (!std::isfinite(tri_n[i])) return bad(err, "non-finite normal in triangle " + std::to_string(i / 3));
    for (int64_t k = 0; k < n_sph; ++k) {
        for (int c = 0; c < 4; ++c)
            if (!std::isfinite(sph[4 * k + c])) return bad(err, "non-finite sphere " + std::to_string(k));
        if (!(sph[4 * k + 3] > 0.0f)) return bad(err, "sphere radius must be > 0");
    }
    return true;
}

bool wide_levels(const float* nodes, int64_t n_nodes, int width, std::vector<int32_t>* list,
                 std::vector<int64_t>* off) {
    const int64_t stride = width == 8 ? kNode8F4 * 4 : kNode4F4 * 4;
    std::vector<int32_t> depth((size_t)std::max<int64_t>(n_nodes, 0), 0);
    int32_t deepest = 0;
    for (int64_t i = 0; i < n_nodes; ++i)
        for (int k = 0; k < width; ++k) {
            int32_t ref;
            std::memcpy(&ref, nodes + i * stride + 6 * width + k, 4);
            if (ref < 0 || ref == 0x7FFFFFFF) continue;   // a leaf, an empty slot
            if (ref <= i || ref >= n_nodes) return false;
            depth[(size_t)ref] = depth[(size_t)i] + 1;
            deepest = std::max(deepest, depth[(size_t)ref]);
        }
    off->assign((size_t)(n_nodes > 0 ? deepest + 2 : 1), 0);
    for (int64_t i = 0; i < n_nodes; ++i) ++(*off)[(size_t)depth[(size_t)i] + 1];
    for (size_t l = 1; l < off->size(); ++l) (*off)[l] += (*off)[l - 1];
    list->assign((size_t)std::max<int64_t>(n_nodes, 0), 0);
    std::vector<int64_t> at(off->begin(), off->end());
    for (int64_t i = 0; i < n_nodes; ++i) (*list)[(size_t)at[(size_t)depth[(size_t)i]]++] = (int32_t)i;
    return true;
}

LbvhScratch lbvh_scratch(int64_t n) {
    const size_t m = (size_t)std::max<int64_t>(n, 1), cap = (size_t)lbvh_node_capacity(n);
    LbvhScratch z;
    z.cen = std::max<size_t>(sizeof(float) * 3 * m, 16);      // centroids
    z.word = std::max<size_t>(sizeof(int32_t) * m, 16);       // codes, ids, sorted codes, splits, first children
    z.key = std::max<size_t>(sizeof(uint64_t) * m, 16);       // sort keys
    z.item = std::max<size_t>(16 * cap, 16);                  // one LbvhItem per node
    z.count = sizeof(int32_t) * (m / 2 + 2);                  // a level's counts and their scan, one word over
    return z;
}

bool LbvhLevels::push(int64_t count, int64_t capacity, int64_t widest) {
    if (count < 0 || count > widest || count > capacity - n_nodes()) return false;
    off.push_back(n_nodes() + count);
    return true;
}

std::vector<int32_t> iota_list(int64_t n_nodes) {
    std::vector<int32_t> v((size_t)std::max<int64_t>(n_nodes, 0));
    for (size_t i = 0; i < v.size(); ++i) v[i] = (int32_t)i;
    return v;
}

long long env_int(const char* name, long long lo, long long hi, long long fallback) {
    const char* v = std::getenv(name);
    return v ? std::max(lo, std::min(hi, std::atoll(v))) : fallback;
}

std::vector<uint32_t> tile_origins(const int32_t* ids, int64_t n, int tiles_x, int tw, int th) {
    std::vector<uint32_t> xy((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        xy[(size_t)i] = ids[i] < 0 ? 0xFFFF0000u
                                   : ((uint32_t)((ids[i] % tiles_x) * tw) << 16) | (uint32_t)((ids[i] / tiles_x) * th);
    return xy;
}

std::vector<int32_t> window_tiles(int W, int x0, int y0, int w, int h, int tw, int th) {
    const int tiles_x = (W + tw - 1) / tw;
    std::vector<int32_t> ids;
    for (int ty = y0 / th; ty <= (y0 + h - 1) / th; ++ty)
        for (int tx = x0 / tw; tx <= (x0 + w - 1) / tw; ++tx) ids.push_back(ty * tiles_x + tx);
    return ids;
}

int latin_stride(int n) {
    int s = std::max(1, (int)std::lround(0.38 * n));
    auto gcd = [](int a, int b) { while (b) { int t = a % b; a = b; b = t; } return a; };
    while (gcd(s, n) != 1) ++s;
    return s;
}

std::vector<std::vector<int32_t>> latin_tile_ids(int W, int H, int tile, int n_ranks) {
    const int tiles_x = (W + tile - 1) / std::max(tile, 1), tiles_y = (H + tile - 1) / std::max(tile, 1);
    const int stride = latin_stride(n_ranks);
    std::vector<std::vector<int32_t>> ids((size_t)n_ranks);
    for (int id = 0; id < tiles_x * tiles_y; ++id)
        ids[(size_t)((id % tiles_x + (int64_t)stride * (id / tiles_x)) % n_ranks)].push_back(id);
    return ids;
}

bool slot_in_frame(const std::vector<uint32_t>& origins, int64_t slot, int tw, int th, int W, int H) {
    const int64_t tpx = (int64_t)tw * th, loc = slot % tpx;
    const uint32_t xy0 = origins[(size_t)(slot / tpx)];
    return (int64_t)(xy0 >> 16) + loc % tw < W && (int64_t)(xy0 & 0xFFFFu) + loc / tw < H;
}

ChunkPlan plan_chunks(int64_t T, int64_t n_slots, int64_t bytes_per_sample, size_t budget) {
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(T, (int64_t)budget / bytes_per_sample));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, ((int64_t)1 << 31) / n_slots - 1));
    const int64_t nc = (T + chunk - 1) / chunk;
    chunk = (T + nc - 1) / nc;
    return ChunkPlan{chunk, (T + chunk - 1) / chunk};
}

FrameSpan launch_frames(int64_t s0, int64_t n, int64_t spp, int64_t n_frames) {
    return FrameSpan{s0 / spp, std::min<int64_t>(n_frames, (s0 + n + spp - 1) / spp)};
}

bool variant_pool(int var) { const Variant* v = find_variant(var); return v && v->pool; }
bool variant_mis(int var) { const Variant* v = find_variant(var); return v && v->mis; }
bool variant_uses_lds(int var) { const Variant* v = find_variant(var); return v && v->lds; }
bool variant_spills(int var) { const Variant* v = find_variant(var); return v && !v->lds; }
bool variant_quantized(int var) { return variant_spills(var); }

int stack_variant(int depth) { return depth + 1 <= 10 ? 10 : depth + 1 <= 16 ? 16 : 32; }

size_t lds_scene_bytes(const LdsSizes& z) {
    LdsSizes scene = z;
    scene.stack = 0;
    return trace_lds(scene).bytes;
}

size_t trace_smem_bytes(int stack, int var, const LdsSizes& z) {
    if (variant_pool(var)) return pool_lds(z).bytes;
    if (!variant_uses_lds(var)) return stack32_bytes(stack);
    LdsSizes own = z;
    own.stack = stack;
    return trace_lds(own).bytes;
}

// LDS-resident scene: BVH + triangles small enough to sit beside the stack
constexpr int64_t kLdsSceneBytes = 24 * 1024;
// ... and whose node indices and leaf references fit the LDS kernels' 16-bit stack entries
// (inner nodes < 0x7FFF, the sentinel; leaf refs >= -32768)
bool lds_fits(const LdsSizes& z) {
    const int64_t n_refs = z.n_tri_f4 / 3;
    return (int64_t)lds_scene_bytes(z) <= kLdsSceneBytes && node_count(z) < 0x7FFF && n_refs * 8 <= 32768;
}

bool variant_takes_width(int var) { const Variant* v = find_variant(var); return v && v->lds && !v->mis; }

// The eight-wide tree: Cornell's 7 BVH4 nodes become 3, a query makes 1.4 visits instead of 3.4, and a
// visit costs two four-wide ones (C2 3.580 -> 3.385 ms per launch, C3 66.5 -> 63.1 ms against the BVH4
// of the same scenes, images identical; DESIGN.md §2, profiles/r13/lds_bvh8/)
constexpr int kLdsWidthDefault = 8;
int lds_width(const LdsSizes& z8, int need8, int knob) {
    const bool can8 = z8.width == 8 && z8.n_node_f4 > 0 && need8 >= 1 && need8 <= 32 && lds_fits(z8);
    if (!can8 || knob == 4) return 4;
    if (knob == 8) return 8;
    LdsSizes own = z8;
    own.stack = need8;
    return pool_lds(own).bytes * 7 <= 160 * 1024 ? kLdsWidthDefault : 4;
}

// LDS-resident scene when it fits; the >= 7 (>= 6) waves/SIMD build when seven (six) blocks'
// LDS still fit one CU (160 KiB), so the occupancy target is not defeated by LDS.
// Everything else (and BVH4s deeper than the 64-entry LDS stack) takes the global-scene
// kernel: 64-B quantised nodes, 16-entry LDS stack + spill, suspended traversal tails,
// >= 6 waves/SIMD (C4: 28.6 ms at 5 waves, 27.2 at 6, 28.6 at 7 with spills).
// An LDS-resident scene whose pooled-shadow kernel still fits seven blocks per CU takes that kernel
// (C2 4.06 vs 4.28 ms, C3 73.6 vs 77.5 ms, profiles/r03/pool/) at every launch size: since round 6
// it also wins the small launches that round 3 left to the phase-aligned kernel (config 1 0.080 vs
// 0.094 ms per launch; DESIGN.md §2, profiles/r06/kernarg/variants/).
// The MIS estimator (PRT_FLAG_MIS_NEE) has one variant per scene placement.
int choose_variant(const LdsSizes& z, int need4, int stack4, bool mis) {
    const bool lds = lds_fits(z) && stack4;
    if (mis) return lds ? kVarLdsMis : kVarGlobalMis;
    if (!lds) return kVarGlobal;
    if (need4 <= 32 && trace_smem_bytes(16, kVarLdsPool, z) * 7 <= 160 * 1024) return kVarLdsPool;
    const size_t smem = trace_smem_bytes(stack4, kVarLds, z);
    return smem * 7 <= 160 * 1024 ? kVarLds : smem * 6 <= 160 * 1024 ? kVarLds6 : kVarLdsAnyOcc;
}

bool camera_is_fast(const float* cam) {
    bool fin = true;
    for (int i = 0; i < 20; ++i) fin = fin && std::isfinite(cam[i]);
    return fin && !(cam[19] > 0.0f) && cam[12] == 0.0f && cam[13] == 0.0f && cam[14] == 0.0f && cam[15] == 1.0f;
}

void camera_terms(const float* cam, float cam_o[3], float cam_k[3]) {
    const float rd2 = -cam[18];
    for (int i = 0; i < 3; ++i) {
        const float* c = cam + 4 * i;
        cam_o[i] = 0.0f * c[0] + 0.0f * c[1] + 0.0f * c[2] + 1.0f * c[3];
        cam_k[i] = rd2 * c[2];
    }
}

}  // namespace prt

#pragma once
// prt_shade.h — launch-parameter access, primary-ray staging and the shading pieces shared by
// trace_kernel, trace_kernel_pool and the hit-query kernels (one copy of each).
#pragma clang fp contract(off)

#include "prt_traverse.h"

namespace prt {
namespace {

// Pixel of work item `item` (slot = tile-major, row, column); xy0 = the item's
// tile origin (x0 << 16 | y0).  Uniform inputs are laundered through SGPR asm so
// the compiler cannot hoist their VALU-derived values out of the persistent loop
// (they would pin VGPRs).
// The kernel's TraceParams in the kernarg segment, through a pointer the compiler cannot follow: every
// field read through it is a scalar load (constant cache) at its use instead of a value held in an
// SGPR across the persistent loop
typedef const __attribute__((address_space(4))) TraceParams KParams;
__device__ __forceinline__ KParams& kernarg() {
    // the kernel's only argument sits at the start of the kernarg segment
    KParams* k = (KParams*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return *k;
}
// trace_kernel: the LDS-scene variants re-read their launch parameters (C1 one-frame launches -13 %,
// C2 -1.5 % against held values spilled into VGPR lanes); the global-scene variant keeps them (C4 +0.8 %
// with re-reads, profiles/r06/kernarg/)
template <bool RELOAD>
__device__ __forceinline__ auto& params(const TraceParams& P) {
    if constexpr (RELOAD) return kernarg();
    else return P;
}
template <class PT>
__device__ __forceinline__ void pixel_of(const PT& P, uint32_t item, uint32_t chunk_s, uint32_t xy0, int& x,
                                         int& y) {
    int log_tw = P.log_tw, log_tpx = P.log_tpx;
    asm volatile("" : "+s"(log_tw), "+s"(log_tpx));
    uint32_t slot = item - chunk_s * (uint32_t)P.n_slots;
    uint32_t loc = slot & ((1u << log_tpx) - 1u);
    x = (int)(xy0 >> 16) + (int)(loc & ((1u << log_tw) - 1u));
    y = (int)(xy0 & 0xFFFFu) + (int)(loc >> log_tw);
}

// Global sample index (the RNG key's sample) of the launch's chunk-relative sample `chunk_s`:
// frame f = j / frame_spp of a multi-frame launch renders samples f * frame_stride + (j % frame_spp)
// (TraceParams::j0).  Wave-uniform operands: one scalar division per chunk or camera wave.
__device__ __forceinline__ uint32_t global_sample(const TraceParams& P, uint32_t chunk_s) {
    uint32_t j = P.j0 + chunk_s, fs = P.frame_spp, st = P.frame_stride, s0 = (uint32_t)P.s0;
    asm volatile("" : "+s"(fs), "+s"(st), "+s"(s0));
    const uint32_t f = j / fs;
    return s0 + f * st + (j - f * fs);
}

// Camera sample for pixel (x, y) of sample `chunk_s` (main_taichi.py:89-95): RNG key,
// jitter, gen_ray.
__device__ __forceinline__ void camera_ray(const TraceParams& P, int x, int y, uint32_t chunk_s, uint32_t& st, V3& o,
                                           V3& d) {
    int W = P.W;
    float wm1 = P.wm1, hm1 = P.hm1;
    asm volatile("" : "+s"(W), "+s"(wm1), "+s"(hm1));
    st = rng_key(P.seed_lo, P.seed_hi, (uint32_t)y * (uint32_t)W + (uint32_t)x, global_sample(P, chunk_s));
    float r0 = rng_next(st);
    float u = ((float)x + r0) / wm1;
    float r1 = rng_next(st);
    float vv = ((float)y + r1) / hm1;
    if (P.cam_fast) {
        // gen_ray for a pinhole affine camera: the same operations minus
        // those with exactly known results (see TraceParams::cam_fast)
        float c[12], k[6];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            c[i] = P.cam[i];
            asm volatile("" : "+s"(c[i]));
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            k[i] = P.cam_o[i];
            k[3 + i] = P.cam_k[i];
            asm volatile("" : "+s"(k[i]), "+s"(k[3 + i]));
        }
        float sd0 = P.cam[16], sd1 = P.cam[17];
        asm volatile("" : "+s"(sd0), "+s"(sd1));
        float rx = (u - 0.5f) * sd0 / 0.5f, ry = (vv - 0.5f) * sd1 / 0.5f;
        float f[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] = (((rx * c[4 * i] + ry * c[4 * i + 1]) + k[3 + i]) + c[4 * i + 3]) - k[i];
        float ln = sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        o = v3(k[0], k[1], k[2]);
        d = v3(f[0] / ln, f[1] / ln, f[2] / ln);
    } else {
        float cam[24];
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            cam[i] = P.cam[i];
            asm volatile("" : "+s"(cam[i]));
        }
        gen_ray(cam, u, vv, st, o, d);
    }
}

// ------------------------------------------------------------------------------------------------
// The work-queue refill of a wave's idle lanes (path regeneration): the chunk claim trace_kernel and
// trace_kernel_pool share.  Each kernel keeps the ballot / rank hand-out around it and the start of an
// item written out (pixel decode, out-of-frame zero write, ray and origin fetch): through a shared
// function the pooled kernel's non-STATS builds spilled 6 to 14 VGPRs where they spill 0 to 2, and the
// global-scene kernel's scratch grew from 28 to 40 bytes (profiles/r12/trace_plumbing/README.md).
// PT: TraceParams or KParams.

// Claims the wave's next chunk [q_next, q_end) of kChunk items from the launch's work counter and
// decodes its sample index and tile origin (both wave-uniform); false: the queue is exhausted.
// PIXEL_MAJOR: the global scenes' chunk order; WAVE_CLOCK: books the items into P.wave_clock
// (trace_kernel's diagnostic).
template <bool PIXEL_MAJOR, bool WAVE_CLOCK, class PT>
__device__ __forceinline__ bool claim_chunk(const PT& Q, int lane, uint32_t& q_next, uint32_t& q_end,
                                            uint32_t& chunk_s, uint32_t& chunk_xy0) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(Q.work, (uint32_t)kChunk);
    base = __builtin_amdgcn_readfirstlane(base);
    if ((uint64_t)base >= Q.n_items) return false;
    if constexpr (PIXEL_MAJOR) {
        // global scenes: queue chunk c -> (sample c % n, 64-pixel group c / n), so
        // the chunks in flight hold every sample of a few pixel groups instead of
        // one sample of the whole frame: their paths start (and first bounce) in a
        // small part of the scene, and its nodes and triangles stay in L2 (C4
        // 18.12 -> 17.51 ms).  LDS scenes keep sample-major chunks, whose staged
        // rays and radiance are read and written in address order (pixel-major
        // there strides 4 MB per chunk: C2 4.23 -> 4.32 ms; profiles/r02/s5/ab_pm/)
        const uint32_t n_samp = (uint32_t)(Q.n_items / (uint64_t)Q.n_slots);
        const uint32_t c = base >> 6;
        const uint32_t g = c / n_samp;
        base = (c - g * n_samp) * (uint32_t)Q.n_slots + (g << 6);
        base = __builtin_amdgcn_readfirstlane(base);
    }
    q_next = base;
    q_end = (uint32_t)min((uint64_t)base + kChunk, Q.n_items);
    if constexpr (WAVE_CLOCK) {
        if (Q.wave_clock && lane == 0)
            Q.wave_clock[3 * ((size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) + 2] += q_end - q_next;
    }
    // n_slots is a multiple of 64 (tile sizes are powers of two >= 64 px),
    // so a chunk never straddles two samples: one scalar division per chunk
    chunk_s = __builtin_amdgcn_readfirstlane(base / (uint32_t)Q.n_slots);
    // tiles hold >= 64 pixels (powers of two), so the chunk lies in one tile
    uint32_t tk = (base - chunk_s * (uint32_t)Q.n_slots) >> Q.log_tpx;
    // uniform index: a scalar load through the constant address space
    chunk_xy0 = ((const __attribute__((address_space(4))) uint32_t*)(uintptr_t)Q.tile_xy)[tk];
    return true;
}

// ------------------------------------------------------------------------------------------------
// Shading and staging pieces shared by trace_kernel, trace_kernel_pool and the hit-query kernels: one
// copy of each, in the reference's expression order (the arithmetic contract).  PT is the launch
// parameters as the caller holds them (TraceParams by value, or KParams through the kernarg pointer);
// PLAIN is the pooled kernel's lean build (triangles and Lambert / emitter materials only).

// The analytic spheres after the triangles of one query (ids n_tri + k), same rule as the oracle:
// closest-hit queries take the nearest root below the triangles' result, any-hit queries (`any`) stop
// at the first sphere hit and skip the loop when a triangle already occludes.
template <class PT>
__device__ __forceinline__ void sphere_hits(const PT& Q, V3 o, V3 d, float tmin, float tmax, bool any, bool& hit,
                                            int& hid, float& ht) {
    if (Q.n_sph > 0 && !(any && hit)) {
        float best = hit ? ht : tmax;
        for (int k = 0; k < Q.n_sph; ++k) {
            float root;
            if (sphere_hit(Q.sph[k], o, d, tmin, best, root)) {
                best = root;
                hid = Q.n_tri + k;
                hit = true;
                if (any) break;
            }
        }
        ht = best;
    }
}

// The surface at hit `hid` (triangle, or sphere n_tri + k: normal (p - c) / r) of the ray (o, d) at ht:
// p = ray.at, the geometric normal, the material row and the normal flipped toward the ray for
// two-sided BSDFs (shapes.py:101-102).
struct Surface { V3 p, ng, n; const float* m; bool flip; };
template <bool PLAIN, class PT>
__device__ __forceinline__ Surface hit_surface(const PT& Q, const float4* s_nm, const float* s_mats, V3 o, V3 d,
                                               float ht, int hid) {
    Surface s;
    s.p = o + d * ht;                                         // ray.at
    int mid;
    if (PLAIN || hid < Q.n_tri) {
        float4 nm = s_nm[hid];
        s.ng = xyz(nm);
        mid = __float_as_int(nm.w);
    } else {                                                   // sphere: (p - c) / r
        asm volatile("");   // keep the divisions in this branch (no if-conversion)
        float4 sc = Q.sph[hid - Q.n_tri];
        s.ng = v3((s.p.x - sc.x) / sc.w, (s.p.y - sc.y) / sc.w, (s.p.z - sc.z) / sc.w);
        mid = Q.sph_mat[hid - Q.n_tri];
    }
    s.m = s_mats + 8 * mid;
    s.flip = s.m[4] == 0.0f && dot(s.ng, neg(d)) < 0.0f;   // shapes.py:101-102
    s.n = s.flip ? neg(s.ng) : s.ng;
    return s;
}

// Specular BSDFs (build-added, config 3; bsdf_taichi.py:52-59, :69-86): metal (type 2) and dielectric
// (type 3), delta distributions.  Returns the scattered direction (not normalised) unless the ray is
// `absorbed`; the caller multiplies beta by the albedo, no NEE.
__device__ __forceinline__ V3 specular_scatter(const float* m, V3 d, V3 ng, uint32_t& st, bool& absorbed) {
    V3 out;
    bool front = dot(d, ng) < 0.0f;
    V3 ns = front ? ng : neg(ng);
    V3 unit = normalize(d);
    absorbed = false;
    if (m[5] == 2.0f) {
        out = reflect3(unit, ns);
        if (m[7] > 0.0f) out = out + random_in_unit_sphere(st) * m[7];
        absorbed = !(dot(out, ns) > 0.0f);
    } else {
        float ratio = front ? 1.0f / m[6] : m[6];
        float ct = -dot(unit, ns);
        ct = ct > 1.0f ? 1.0f : ct;
        float stn = sqrtf(1.0f - ct * ct);
        bool cannot = ratio * stn > 1.0f;
        if (cannot || schlick(ct, ratio) > rng_next(st)) out = reflect3(unit, ns);
        else out = refract3(unit, ns, ratio);
    }
    return out;
}

// The local direction l in the hit's shading frame (shapes.py:105-108).  Triangles read rotate_z_to's
// rows precomputed on the host with the same f32 arithmetic (per face and side); spheres build them here.
template <bool PLAIN, class PT>
__device__ __forceinline__ const float4* frame_rows(const PT& Q, const float4* s_fr, int hid, bool flip) {
    return s_fr + ((size_t)((PLAIN || hid < Q.n_tri) ? hid : 0) * 2 + (flip ? 1 : 0)) * 3;
}
template <bool FAST, bool PLAIN, class PT>
__device__ __forceinline__ V3 frame_dir(const PT& Q, const float4* fr, int hid, V3 n, V3 l) {
    if (PLAIN || hid < Q.n_tri) {
        float4 f0 = fr[0], f1 = fr[1], f2 = fr[2];
        return normalize<FAST>(xyz(f0) * l.x + xyz(f1) * l.y + xyz(f2) * l.z);
    }
    return to_world(n, l);
}

// BSDFLambertian.scatter + frame (bsdf.py:29-34): the cosine-weighted direction wi in the hit's frame fr
template <bool FAST, bool PLAIN, class PT>
__device__ __forceinline__ V3 lambert_dir(const PT& Q, const float4* fr, int hid, V3 n, uint32_t& st) {
    float u0 = rng_next(st);
    float u1 = rng_next(st);
    V3 l = cosine_hemisphere<FAST>(u0, u1);
    return frame_dir<FAST, PLAIN>(Q, fr, hid, n, l);
}
// ... and the path weight's factor att * max(cw, 0) / pdf * InvPi for it (m: the material row)
template <bool FAST>
__device__ __forceinline__ V3 lambert_weight(const float* m, V3 n, V3 wi, int shade_fast) {
    float pdf = fabsf(dot(n, wi)) * kInvPi;
    V3 att = v3(m[0], m[1], m[2]);
    float cw = dot(n, wi);
    float dz = cw > 0.0f ? cw : 0.0f;
    // tracing.py:146-148: if any component of att*dz/pdf*InvPi is NaN the
    // reference recomputes it with pdf = 1e-4.  (a / pdf) * InvPi is NaN
    // exactly when a / pdf is, so the condition is decided before dividing.
    V3 ad = v3(att.x * dz, att.y * dz, att.z * dz);
    V3 adp = lambert_div<FAST>(ad, pdf, cw, shade_fast);
    return v3(adp.x * kInvPi, adp.y * kInvPi, adp.z * kInvPi);
}

// sample_direct_lighting's light-triangle sample (tracing.py:92-108): a light, one of its triangles
// (v0, v1, v2; nm = normal xyz, material id bits) and the point p2 on it.
struct LightSample { float4 v0, v1, v2, nm; V3 p2; };
template <bool FAST, class PT>
__device__ __forceinline__ LightSample sample_light(const PT& Q, const int* s_loff, const float4* s_lv, uint32_t& st) {
    int li = Q.n_light > 1 ? rng_int(st, 0, Q.n_light - 1) : 0;
    int lo = s_loff[li];
    int f = rng_int(st, 0, s_loff[li + 1] - lo - 1);
    float su = sqrt_cr<FAST>(rng_next(st));
    float sv = rng_next(st);
    float a = su * (1.0f - sv);
    float b = su * sv;
    const float4* lv = s_lv + (size_t)(lo + f) * 4;
    LightSample ls;
    ls.v0 = lv[0]; ls.v1 = lv[1]; ls.v2 = lv[2]; ls.nm = lv[3];
    float c = 1.0f - a - b;
    ls.p2 = (xyz(ls.v0) * a + xyz(ls.v1) * b) + xyz(ls.v2) * c;
    return ls;
}

// The NEE shadow ray from p (normal n) to the light sample p2 (normal n2): direction w, the reference's
// bound t_at_light and the two cosines; the term is possible when both are positive.
struct NeeRay { V3 w; float t_at, dot1, dot2; };
template <bool FAST>
__device__ __forceinline__ NeeRay nee_ray(V3 p, V3 n, V3 p2, V3 n2) {
    NeeRay r;
    r.w = normalize<FAST>(p2 - p);
    r.t_at = (p2.x - p.x) / r.w.x;
    // w2 = normalize(p - p2) is -w bit for bit (round-to-nearest is sign
    // symmetric) up to the sign of zero components, so dot(n2, w2) =
    // -dot(n2, w) except for the sign of a zero result, which the
    // strict "> 0" test and the uses below cannot see.
    r.dot1 = dot(n, r.w);
    r.dot2 = -dot(n2, r.w);
    return r;
}
// ... and its radiance em * dot1 * dot2 / |p - p2|^2 for the emitter's material row em (the caller
// weights it by beta)
template <bool FAST>
__device__ __forceinline__ V3 nee_radiance(const float* em, V3 p, V3 p2, float dot1, float dot2, int shade_fast) {
    V3 dd = p - p2;
    float sl = dot(dd, dd);
    return nee_div<FAST>(v3(em[0] * dot1 * dot2, em[1] * dot1 * dot2, em[2] * dot1 * dot2), sl, dot1, dot2,
                         shade_fast);
}

// A finished sample: its radiance to out[item] and the lane freed.
template <bool STATS, class PT>
__device__ __forceinline__ void finish_sample(const PT& Q, int& item, V3 L, Counters& cn) {
    float* out = Q.out + (size_t)item * 3;
    out[0] = L.x; out[1] = L.y; out[2] = L.z;
    // failure detection (STATS): samples whose radiance is NaN or infinite
    if (STATS && !(isfinite(L.x) && isfinite(L.y) && isfinite(L.z))) cn.nonfinite++;
    item = -1;
}

// STATS epilogues: a wave's sum / maximum of v, valid in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_down((int)v, off));
    return v;
}

// Block copy of an LDS-resident scene's BVH4 as 8 octant copies per node (visit_node4 OCT): copy
// k of node n holds the near / far planes of each axis for the direction signs k = sx | sy << 1 |
// sz << 2, then the refs with the empty-slot reference rewritten to the 16-bit stack's sentinel,
// the four children in k's front-to-back order (ascending near corner along the octant's
// diagonal, empty slots last, ties by index).
__device__ __forceinline__ void copy_octant_nodes(float4* __restrict__ sn, const float4* __restrict__ nodes,
                                                  int n_node4) {
    for (int i = threadIdx.x; i < 56 * n_node4; i += kBlock) {
        const int n = i / 56, r = i - 56 * n, k = r / 7, slot = r - 7 * k;
        const int ax = slot >> 1, sgn = (k >> ax) & 1, far = slot & 1;
        const float4* src = nodes + 8 * n;
        float4 v = slot == 6 ? src[6] : src[2 * ax + (sgn ^ far)];
        if (slot == 6) {
            int* rr = reinterpret_cast<int*>(&v);
            for (int c = 0; c < 4; ++c) rr[c] = rr[c] == kSentinel ? kSentinel16 : rr[c];
        }
        // copy k orders the children front to back for its direction signs (visit_node4 OCT):
        // ascending near corner along the octant's diagonal, empty slots last, ties by index
        float key[4];
        {
            const float4 lx = src[0], hx = src[1], ly = src[2], hy = src[3], lz = src[4], hz = src[5];
            const float4 rf = src[6];
            const int rr[4] = {__float_as_int(rf.x), __float_as_int(rf.y), __float_as_int(rf.z), __float_as_int(rf.w)};
            // near corner of the box, projected on the octant's diagonal
            const float nxv[4] = {lx.x, lx.y, lx.z, lx.w}, fxv[4] = {hx.x, hx.y, hx.z, hx.w};
            const float nyv[4] = {ly.x, ly.y, ly.z, ly.w}, fyv[4] = {hy.x, hy.y, hy.z, hy.w};
            const float nzv[4] = {lz.x, lz.y, lz.z, lz.w}, fzv[4] = {hz.x, hz.y, hz.z, hz.w};
            for (int c = 0; c < 4; ++c) {
                key[c] = rr[c] == kSentinel ? INFINITY
                                            : ((k & 1) ? -fxv[c] : nxv[c]) + ((k & 2) ? -fyv[c] : nyv[c]) +
                                                  ((k & 4) ? -fzv[c] : nzv[c]);
                if (!(key[c] == key[c])) key[c] = INFINITY;   // NaN (degenerate box): a total order
            }
        }
        const float vin[4] = {v.x, v.y, v.z, v.w};
        int rank[4];   // position of child c in the order (a permutation of 0..3)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            rank[c] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) rank[c] += (key[e] < key[c] || (key[e] == key[c] && e < c)) ? 1 : 0;
        }
        // slot j takes the child of rank j (selects, no dynamically indexed array in scratch)
        float vout[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            vout[j] = rank[0] == j ? vin[0] : rank[1] == j ? vin[1] : rank[2] == j ? vin[2] : vin[3];
        sn[i] = make_float4(vout[0], vout[1], vout[2], vout[3]);
    }
}

// The same for an LDS-resident scene's BVH8 (prt_internal.h Bvh8Host; visit_node8): copy k of node n is
// 14 float4 — the near / far planes of each axis for children 0-3 of k's front-to-back order, the same six
// for children 4-7, then the eight refs as two quads; node stride 112 float4.  The order is
// copy_octant_nodes' (ascending near corner along the octant's diagonal, empty slots last, ties by index).
__device__ __forceinline__ void copy_octant_nodes8(float4* __restrict__ sn, const float4* __restrict__ nodes,
                                                   int n_node8) {
    for (int i = threadIdx.x; i < 112 * n_node8; i += kBlock) {
        const int n = i / 112, r = i - 112 * n, k = r / 14, slot = r - 14 * k;
        const float4* src = nodes + 14 * n;
        const bool refs = slot >= 12;
        const int g = refs ? slot - 12 : slot / 6;        // the group of four output children
        // plane slots: the source plane of axis ax, near or far for the octant's sign (refs: unused, 0)
        const int s6 = refs ? 0 : slot - 6 * g, ax = s6 >> 1, sgn = (k >> ax) & 1, far = s6 & 1;
        const int plane = 2 * ax + (sgn ^ far);
        const float4 va = refs ? src[12] : src[plane], vb = refs ? src[13] : src[6 + plane];
        float vin[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
        const float4 ra = src[12], rb = src[13];
        const int rr[8] = {__float_as_int(ra.x), __float_as_int(ra.y), __float_as_int(ra.z), __float_as_int(ra.w),
                           __float_as_int(rb.x), __float_as_int(rb.y), __float_as_int(rb.z), __float_as_int(rb.w)};
        if (refs) {
#pragma unroll
            for (int c = 0; c < 8; ++c) vin[c] = rr[c] == kSentinel ? __int_as_float(kSentinel16) : vin[c];
        }
        // near corner of each box, projected on the octant's diagonal
        float key[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4* q = src + 6 * h;
            const float4 cx = (k & 1) ? q[1] : q[0], cy = (k & 2) ? q[3] : q[2], cz = (k & 4) ? q[5] : q[4];
            const float xs[4] = {cx.x, cx.y, cx.z, cx.w}, ys[4] = {cy.x, cy.y, cy.z, cy.w};
            const float zs[4] = {cz.x, cz.y, cz.z, cz.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v = ((k & 1) ? -xs[c] : xs[c]) + ((k & 2) ? -ys[c] : ys[c]) + ((k & 4) ? -zs[c] : zs[c]);
                if (rr[4 * h + c] == kSentinel || !(v == v)) v = INFINITY;   // NaN (degenerate box): a total order
                key[4 * h + c] = v;
            }
        }
        int rank[8];   // position of child c in the order (a permutation of 0..7)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            rank[c] = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) rank[c] += (key[e] < key[c] || (key[e] == key[c] && e < c)) ? 1 : 0;
        }
        // output child j of the group takes the child of rank 4 g + j (selects, no indexed array in scratch)
        float vout[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = vin[7];
#pragma unroll
            for (int c = 6; c >= 0; --c) v = rank[c] == 4 * g + j ? vin[c] : v;
            vout[j] = v;
        }
        sn[i] = make_float4(vout[0], vout[1], vout[2], vout[3]);
    }
}
// the block's octant copy of the tree of W children per node
template <int W>
__device__ __forceinline__ void copy_octant_tree(float4* __restrict__ sn, const float4* __restrict__ nodes,
                                                 int n_node_f4) {
    if constexpr (W == 8) copy_octant_nodes8(sn, nodes, n_node_f4 / 14);
    else copy_octant_nodes(sn, nodes, n_node_f4 / 8);
}

}  // namespace
}  // namespace prt

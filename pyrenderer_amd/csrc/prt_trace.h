#pragma once
// prt_trace.h — trace_kernel, the persistent per-wave trace kernel (LDS-resident and global scenes,
// NEE and MIS estimators).
#pragma clang fp contract(off)

#include <type_traits>

#include "prt_shade.h"

namespace prt {
namespace {

enum : int { Q_EXT = 0, Q_SHADOW = 1, Q_MISL = 2, Q_MISB = 3 };

// MIS direct-lighting variant (trace_kernel's MIS): the reference's unused estimator
// PathTracer.sample_direct_lighting2 and its helpers (core/tracing.py:12-90), restated
// as oracle/prt_oracle.c:direct_mis.  Both strategies' visibility tests are closest-hit
// queries over (1e-5, 9999.9) that must land on an emitter; light_area = 1.0 and the
// BRDF strategy's light pdf uses the light-sampled point's normal, as the reference has it.
constexpr float kTMaxMis = 9999.9f;
constexpr float kPiF = 3.14159265358979323846f;   // np.pi inside a Taichi f32 kernel
__device__ __forceinline__ float dot_or_zero(V3 n, V3 l) { float d = dot(n, l); return 0.0f > d ? 0.0f : d; }
__device__ __forceinline__ float mis_power(float pf, float pg) {
    float f = pf * pf, g = pg * pg;
    return f / (f + g);
}
__device__ __forceinline__ float area_light_pdf(float t_light, V3 dir, V3 light_n) {
    float pdf = 0.0f;
    float l_cos = dot(light_n, neg(dir));
    if (l_cos > 1e-4f) {
        V3 tmp = dir * t_light;
        pdf = dot(tmp, tmp) / (1.0f * l_cos);
    }
    return pdf;
}

// Two things vary besides STACK, STATS and the occupancy target WPE; the traversal is always the
// while-while BVH4 (traverse_ww4):
//   SCENE_LDS  the scene (octant BVH4 copies, triangles, shading data) sits in the block's LDS, the
//              traversal stacks hold 16-bit entries, and the shading sqrt and quotients take their
//              fast paths (sqrt_cr; lambert_div, nee_div: in the global-scene kernel, which is L1-bound,
//              the cheap guards measured +0.3 % at C4, profiles/r06/guards/ab_c4_global_fastdiv.jsonl).
//              Otherwise the scene stays in global memory as quantised 64-B nodes, the stack is STACK
//              LDS entries plus a global spill area, and traversal tails are suspended and resumed in
//              the next iteration.
//   MIS        MIS direct lighting (sample_direct_lighting2) instead of NEE.
//   BW         children per node of the LDS-resident tree of the phase-aligned kernels (4, or 8: the BVH8);
//              the MIS and global-scene kernels exist for 4 only.
template <int STACK, bool STATS, bool SCENE_LDS, bool MIS, int WPE, int BW>
__global__ __attribute__((amdgpu_flat_work_group_size(kBlock, kBlock), amdgpu_waves_per_eu(WPE)))
void trace_kernel(TraceParams P) {
    // phase-aligned scheduling (see below): the LDS scenes' NEE kernels; the MIS estimator's three query
    // kinds and the global scenes' suspended queries keep the mixed schedule
    constexpr bool PHASE = SCENE_LDS && !MIS;
    static_assert(BW == 4 || (BW == 8 && PHASE), "only the phase-aligned LDS kernels traverse the eight-wide tree");
    extern __shared__ float4 smem[];
    // LDS: the traversal stacks (16-bit entries for LDS-resident scenes), then the scene copy
    using StackT = typename std::conditional<SCENE_LDS, LdsStack16A, SpillStack<STACK>>::type;
    StackT stk;
    if constexpr (SCENE_LDS) {
        stk = LdsStack16A::at(smem, threadIdx.x);
    } else {
        stk.l = reinterpret_cast<int*>(smem) + threadIdx.x;
        stk.g = P.spill + (size_t)blockIdx.x * kBlock + threadIdx.x;
        stk.gs = gridDim.x * kBlock;
    }
    const float4* g_nodes = P.nodes;
    const float4* g_tris = P.tris;
    const float4* s_nm = P.tri_nm;
    const float4* s_fr = P.tri_frame;
    const float* s_mats = P.mats;
    const float4* s_lv = P.light_v;
    const int* s_loff = P.light_off;
    if (SCENE_LDS) {
        // small scene: copy BVH + triangles, and the shading data (normals, frames,
        // materials, emitters), into LDS once per persistent block (layout: prt_lds_layout.h)
        const TraceLds lay = trace_lds(lds_sizes(P, STACK, BW));
        float4* sn = smem + lay.nodes;
        float4* st4 = smem + lay.tris;
        float4* snm = smem + lay.normals;
        float4* sfr = smem + lay.frames;
        float4* smt = smem + lay.mats;
        float4* slv = smem + lay.light_v;
        int* slo = reinterpret_cast<int*>(smem + lay.light_off);
        copy_octant_tree<BW>(sn, P.nodes, P.n_node_f4);
        for (int i = threadIdx.x; i < P.n_tri_f4; i += kBlock) st4[i] = P.tris[i];
        for (int i = threadIdx.x; i < P.n_tri; i += kBlock) snm[i] = P.tri_nm[i];
        for (int i = threadIdx.x; i < 6 * P.n_tri; i += kBlock) sfr[i] = P.tri_frame[i];
        for (int i = threadIdx.x; i < 2 * P.n_mat; i += kBlock) smt[i] = reinterpret_cast<const float4*>(P.mats)[i];
        for (int i = threadIdx.x; i < 4 * P.n_lt; i += kBlock) slv[i] = P.light_v[i];
        for (int i = threadIdx.x; i <= P.n_light; i += kBlock) slo[i] = P.light_off[i];
        __syncthreads();
        g_nodes = sn;
        g_tris = st4;
        s_nm = snm;
        s_fr = sfr;
        s_mats = reinterpret_cast<const float*>(smt);
        s_lv = slv;
        s_loff = slo;
    }
    const int lane = threadIdx.x & 63;
    // diagnostic (P.wave_clock, env PRT_WAVE_CLOCK): each wave's start / end real time and the
    // items it took, kept in memory (not registers: the hot loop's VGPR budget is tight)
    if (P.wave_clock && lane == 0)
        P.wave_clock[3 * ((size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6))] = __builtin_amdgcn_s_memrealtime();

    // wave-uniform work queue [q_next, q_end)
    uint32_t q_next = 0, q_end = 0;
    bool exhausted = false;

    // lane state
    TState tst = {0, 0, 0, -1, 0.0f};
    bool pending = false;   // global scenes: a suspended query (state in tst + the LDS stack)
    int item = -1;
    int bounce = 0, qtype = Q_EXT;
    uint32_t st = 0;
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0), wi = v3(0, 0, 0);
    V3 beta = v3(1, 1, 1), L = v3(0, 0, 0), pend = v3(0, 0, 0);
    // MIS: shading normal, light-sampled point's normal, InvPi * rho * light colour, the
    // BRDF-strategy direction and pdf of the current vertex (pend accumulates direct_li)
    V3 mis_n = v3(0, 0, 0), mis_n2 = v3(0, 0, 0), mis_fl = v3(0, 0, 0), mis_bd = v3(0, 0, 0);
    float mis_bp = 0.0f;
    float tmax = kTMax;
    Counters cn = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t w_inner = 0, w_leaf = 0, l_inner = 0, l_leaf = 0;
    uint32_t chunk_s = 0;   // wave-uniform: sample index (within the launch) of the current chunk
    uint32_t chunk_xy0 = 0; // wave-uniform: origin of the current chunk's tile

    // diagnostic (STATS) wave-level clocks: refill / traversal / shading, iterations, active lanes
    uint64_t c_refill = 0, c_trav = 0, c_shade = 0, n_iter = 0, n_active = 0;
    // STATS, phase-aligned schedule: wave clocks and counts of extension / shadow iterations and the
    // lanes that queried in the shadow ones (PRT_DIAG_PHASE)
    uint64_t c_it_ext = 0, c_it_sh = 0, n_it_ext = 0, n_it_sh = 0, lanes_sh = 0, t_it = 0;
    uint64_t t_a = 0, t_b = 0;
    // PHASE: the wave alternates extension and shadow iterations, so the costly
    // shading code (run after extension queries only) and the refill execute
    // with every busy lane at once instead of every iteration with about half.
    // Lanes whose query kind does not match the wave's phase sit the iteration out.
    bool last_shadow = false;
    while (true) {
        // LDS scenes: launch parameters re-read through the kernarg pointer each iteration (see params)
        auto& Q = params<SCENE_LDS>(P);
        if (STATS) { t_a = __builtin_amdgcn_s_memtime(); t_it = t_a; }
        bool do_shadow = false;
        if (PHASE) {
            do_shadow = !last_shadow && __ballot(item >= 0 && qtype == Q_SHADOW) != 0;
            last_shadow = do_shadow;
        }
        // ---------------------------------------------------------- refill
        // me_idle: this lane's own bit of `idle` (kept as a lane predicate: testing the bit
        // needs the 64-bit mask 1 << lane, which the register allocator spilled to scratch)
        bool me_idle = !do_shadow && item < 0;
        uint64_t idle = __ballot(me_idle);
        for (int round = 0; round < 2 && idle; ++round) {
            uint32_t avail = q_end - q_next;
            if (avail == 0 && !exhausted) {
                // global scenes take pixel-major chunks (claim_chunk)
                exhausted = !claim_chunk<!SCENE_LDS, true>(Q, lane, q_next, q_end, chunk_s, chunk_xy0);
                avail = q_end - q_next;
            }
            if (avail == 0) break;
            uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            uint32_t need = (uint32_t)__popcll(idle);
            uint32_t take = need < avail ? need : avail;
            if (me_idle && rank < take) {
                item = (int)(q_next + rank);
                // start a new sample (main_taichi.py:89-95).  Written out here and in trace_kernel_pool:
                // as a function shared by both, the pooled, global-scene and MIS kernels spilled more
                // (prt_shade.h at claim_chunk; profiles/r12/trace_plumbing/README.md)
                L = v3(0, 0, 0);
                int x, y;
                pixel_of(Q, (uint32_t)item, chunk_s, chunk_xy0, x, y);
                int W = Q.W, H = Q.H;
                asm volatile("" : "+s"(W), "+s"(H));
                bool ok = x < W && y < H;
                if (ok) {
                    // primary rays from camera_kernel (or prt_trace_rays' caller rays): no camera code
                    // in the persistent loop, whose uniform operands would spill SGPRs
                    float4 r = Q.rays[item];
                    d = v3(r.x, r.y, r.z);
                    st = __float_as_uint(r.w);
                    if (Q.ray_o) {
                        // per-ray origins: prt_trace_rays' caller rays, thin-lens / projective cameras
                        const float4 ro = Q.ray_o[item];
                        o = v3(ro.x, ro.y, ro.z);
                    } else {
                        float o0 = Q.cam_o[0], o1 = Q.cam_o[1], o2 = Q.cam_o[2];
                        asm volatile("" : "+s"(o0), "+s"(o1), "+s"(o2));
                        o = v3(o0, o1, o2);
                    }
                }
                if (!ok) {
                    float* out = Q.out + (size_t)item * 3;
                    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
                    item = -2;  // served, nothing to trace this iteration
                } else {
                    beta = v3(1, 1, 1);
                    bounce = 0;
                    qtype = Q_EXT;
                    tmax = kTMax;
                }
            }
            q_next += take;
            me_idle = item == -1;
            idle = __ballot(me_idle);
        }
        if (item == -2) item = -1;
        if (__ballot(item >= 0) == 0) {
            if (exhausted && q_next == q_end) break;
            continue;
        }
        if (item < 0) continue;
        if (PHASE && (qtype == Q_SHADOW) != do_shadow) continue;

        // ------------------------------------------------------- one query
        int hid = -1;
        float ht = 0.0f;
        bool hit;
        if (STATS) {
            if (!pending) {
                if (qtype == Q_EXT) cn.ext++; else cn.shadow++;
            }
            // wave-level clocks: the first active lane books the interval
            const bool leader = __builtin_amdgcn_readfirstlane(lane) == lane;
            const uint64_t active = __ballot(true);
            t_b = __builtin_amdgcn_s_memtime();
            if (leader) {
                c_refill += t_b - t_a;
                n_iter++;
                n_active += (uint64_t)__popcll(active);
                if (PHASE && do_shadow) lanes_sh += (uint64_t)__popcll(active);
            }
            t_a = t_b;
        }
        // the leaf-phase entry / exit thresholds (counts of lanes) are tuned for full waves; in
        // the drain, with few lanes left, they would switch phase after every trip
        const int lb = exhausted ? 0 : Q.leaf_break, le = exhausted ? 0 : Q.leaf_exit;
        const uint32_t glim = Q.guard_trips;
        if (STATS && !pending) cn.q0 = cn.nodes;   // node visits at the start of this query
        if constexpr (!SCENE_LDS) {
            if (!pending) tstate_init(tst, stk, tmax);
            // suspending a query only pays while idle lanes can be refilled: once the work
            // queue is exhausted (the launch's drain) the wave keeps traversing instead of
            // going round the loop once per inner/leaf phase
            const int res_min = exhausted ? 0 : Q.resume_min;
            // mixed query kinds over quantised nodes, resumable
            const bool done = traverse_ww4<STATS, 0, StackT, true, true>(g_nodes, g_tris, o, d, kTMin, tmax,
                                                                         qtype == Q_SHADOW, stk, hid, ht, cn, &tst,
                                                                         res_min, Q.fault, lb, le, glim);
            pending = !done;
            if (pending) continue;   // resume next iteration; no shading yet
            hit = hid >= 0;
        } else if (PHASE) {
            if (do_shadow)
                hit = traverse_ww4<STATS, 2, StackT, false, false, true, BW>(g_nodes, g_tris, o, d, kTMin, tmax, true, stk,
                                                                         hid, ht, cn, nullptr, 0, Q.fault, lb, le, glim);
            else
                hit = traverse_ww4<STATS, 1, StackT, false, false, true, BW>(g_nodes, g_tris, o, d, kTMin, tmax, false, stk,
                                                                         hid, ht, cn, nullptr, 0, Q.fault, lb, le, glim);
        } else {
            // LDS scene, MIS: the mixed schedule (closest-hit queries of three kinds)
            hit = traverse_ww4<STATS, 0, StackT, false, false, true>(g_nodes, g_tris, o, d, kTMin, tmax,
                                                                     qtype == Q_SHADOW, stk, hid, ht, cn, nullptr, 0,
                                                                     Q.fault, lb, le, glim);
        }

        if (STATS) {
            const uint32_t qn = cn.nodes - cn.q0;
            cn.max_q = max(cn.max_q, qn);   // most node visits of one query
            // outlier log (PRT_DIAG_OUTLIER_LOG): the first 16 queries with > 1000 node visits
            if (qn > 1000) {
                const unsigned long long k = atomicAdd(Q.stats + PRT_DIAG_OUTLIERS, 1ull);
                if (k < PRT_DIAG_OUTLIER_RECORDS) {
                    unsigned long long* r = Q.stats + PRT_DIAG_OUTLIER_LOG + PRT_DIAG_OUTLIER_WORDS * k;
                    r[0] = __float_as_uint(o.x); r[1] = __float_as_uint(o.y); r[2] = __float_as_uint(o.z);
                    r[3] = __float_as_uint(d.x); r[4] = __float_as_uint(d.y); r[5] = __float_as_uint(d.z);
                    r[6] = __float_as_uint(tmax); r[7] = ((unsigned long long)qtype << 32) | qn;
                }
            }
        }
        if (Q.n_sph > 0 && !(qtype == Q_SHADOW && hit)) {
            // analytic spheres after the triangles (ids n_tri + k), same rule as the oracle
            float best = hit ? ht : tmax;
            for (int k = 0; k < Q.n_sph; ++k) {
                float root;
                if (sphere_hit(Q.sph[k], o, d, kTMin, best, root)) {
                    best = root;
                    hid = Q.n_tri + k;
                    hit = true;
                    if (qtype == Q_SHADOW) break;
                }
            }
            ht = best;
        }
        if (STATS) {
            const bool leader = __builtin_amdgcn_readfirstlane(lane) == lane;
            t_b = __builtin_amdgcn_s_memtime();
            if (leader) c_trav += t_b - t_a;
            t_a = t_b;
            // wave-level loop trips = max over the participating lanes; lane-level = sum
            uint32_t mi = cn.it_inner, ml = cn.it_leaf;
            for (int off = 32; off > 0; off >>= 1) {
                mi = max(mi, (uint32_t)__shfl_xor((int)mi, off));
                ml = max(ml, (uint32_t)__shfl_xor((int)ml, off));
            }
            if (leader) { w_inner += mi; w_leaf += ml; }
            l_inner += cn.it_inner; l_leaf += cn.it_leaf;
            cn.it_inner = 0; cn.it_leaf = 0;
        }
        // ------------------------------------------------- shade the result
        bool finished = false;
        if (qtype == Q_EXT) {
            if (!hit) {
                finished = true;
            } else {
                const Surface sf = hit_surface<false>(Q, s_nm, s_mats, o, d, ht, hid);
                const V3 p = sf.p, ng = sf.ng, n = sf.n;
                const float* m = sf.m;
                const bool flip = sf.flip;
                if (m[5] == 2.0f || m[5] == 3.0f) {
                    bool absorbed;
                    const V3 out = specular_scatter(m, d, ng, st, absorbed);
                    if (absorbed) {
                        finished = true;
                    } else {
                        beta = beta * v3(m[0], m[1], m[2]);
                        o = p;
                        d = normalize(out);
                        ++bounce;
                        if (bounce >= Q.depth) finished = true;
                    }
                } else if (m[3] != 0.0f) {                                 // tracing.py:129-139
                    float d1 = dot(neg(d), n);
                    if (d1 > 0.0f) {
                        V3 lc = v3(Q.dl_r, Q.dl_g, Q.dl_b);
                        L = bounce == 0 ? L + lc * beta : L + (lc * beta) * d1;
                    }
                    finished = true;
                } else {
                    // BSDFLambertian.scatter + frame (bsdf.py:29-34, shapes.py:105-108)
                    const float4* fr = frame_rows<false>(Q, s_fr, hid, flip);
                    wi = lambert_dir<SCENE_LDS, false>(Q, fr, hid, n, st);
                    beta = beta * lambert_weight<SCENE_LDS>(m, n, wi, Q.shade_fast);
                    const LightSample ls = sample_light<SCENE_LDS>(Q, s_loff, s_lv, st);
                    const float4 LN = ls.nm;
                    const V3 p2 = ls.p2, n2 = xyz(LN);
                    if constexpr (MIS) {
                        // sample_direct_lighting2: the BRDF strategy's direction is drawn now
                        // (queries draw nothing, so the stream order is the reference's)
                        const float* em = s_mats + 8 * __float_as_int(LN.w);
                        mis_fl = v3(m[0] * kInvPi * em[0], m[1] * kInvPi * em[1], m[2] * kInvPi * em[2]);
                        V3 tl = normalize<SCENE_LDS>(p2 - p);
                        float b0 = rng_next(st);
                        float b1 = rng_next(st);
                        V3 bl = cosine_hemisphere<SCENE_LDS>(b0, b1);
                        mis_bd = frame_dir<SCENE_LDS, false>(Q, fr, hid, n, bl);
                        mis_bp = fabsf(dot(n, mis_bd)) * kInvPi;
                        mis_n = n;
                        mis_n2 = n2;
                        pend = v3(0, 0, 0);
                        o = p;
                        tmax = kTMaxMis;
                        if (dot(tl, n) > 0.0f) {
                            d = tl;
                            qtype = Q_MISL;
                        } else if (mis_bp > 0.0f) {
                            d = mis_bd;
                            qtype = Q_MISB;
                        } else {
                            L = L + beta * pend;
                            ++bounce;
                            if (bounce >= Q.depth) finished = true;
                            d = wi;
                            tmax = kTMax;
                        }
                    } else {
                        // sample_direct_lighting (tracing.py:92-108)
                        const NeeRay nr = nee_ray<SCENE_LDS>(p, n, p2, n2);
                        o = p;
                        if (nr.dot1 > 0.0f && nr.dot2 > 0.0f) {
                            const float* em = s_mats + 8 * __float_as_int(LN.w);
                            pend = beta * nee_radiance<SCENE_LDS>(em, p, p2, nr.dot1, nr.dot2, Q.shade_fast);
                            d = nr.w;
                            tmax = nr.t_at;
                            qtype = Q_SHADOW;
                        } else {
                            // no NEE term possible: go straight to the next bounce
                            ++bounce;
                            if (bounce >= Q.depth) finished = true;
                            d = wi;
                            tmax = kTMax;
                        }
                    }
                }
            }
        } else if (MIS && qtype == Q_MISL) {
            // light strategy: visible when the closest hit is an emitter
            if (hit) {
                const int mid = hid < Q.n_tri ? __float_as_int(s_nm[hid].w) : Q.sph_mat[hid - Q.n_tri];
                if (s_mats[8 * mid + 3] > 0.0f) {
                    float lp = area_light_pdf(ht, d, mis_n2);
                    float bp = dot_or_zero(mis_n, d) / kPiF;
                    if (lp > 0.0f && bp > 0.0f) {
                        float w = mis_power(lp, bp);
                        float nl = dot_or_zero(d, mis_n);
                        pend = pend + v3(mis_fl.x * w * nl / lp, mis_fl.y * w * nl / lp, mis_fl.z * w * nl / lp);
                    }
                }
            }
            if (mis_bp > 0.0f) {
                d = mis_bd;          // o is still the vertex, tmax kTMaxMis
                qtype = Q_MISB;
            } else {
                L = L + beta * pend;
                ++bounce;
                if (bounce >= Q.depth) finished = true;
                d = wi;
                tmax = kTMax;
                qtype = Q_EXT;
            }
        } else if (MIS && qtype == Q_MISB) {
            // BRDF strategy
            if (hit) {
                const int mid = hid < Q.n_tri ? __float_as_int(s_nm[hid].w) : Q.sph_mat[hid - Q.n_tri];
                if (s_mats[8 * mid + 3] > 0.0f) {
                    float lp = area_light_pdf(ht, d, mis_n2);
                    if (lp > 0.0f) {
                        float w = mis_power(mis_bp, lp);
                        float nl = dot_or_zero(d, mis_n);
                        pend = pend + v3(mis_fl.x * w * nl / mis_bp, mis_fl.y * w * nl / mis_bp,
                                         mis_fl.z * w * nl / mis_bp);
                    }
                }
            }
            L = L + beta * pend;
            ++bounce;
            if (bounce >= Q.depth) finished = true;
            d = wi;
            tmax = kTMax;
            qtype = Q_EXT;
        } else {
            if (!hit) L = L + pend;
            ++bounce;
            if (bounce >= Q.depth) finished = true;
            d = wi;           // o is still the hit point p
            tmax = kTMax;
            qtype = Q_EXT;
        }
        if (finished) finish_sample<STATS>(Q, item, L, cn);
        if (STATS) {
            const bool leader = __builtin_amdgcn_readfirstlane(lane) == lane;
            if (leader) {
                const uint64_t t_end = __builtin_amdgcn_s_memtime();
                c_shade += t_end - t_a;
                if (do_shadow) { c_it_sh += t_end - t_it; n_it_sh++; }
                else { c_it_ext += t_end - t_it; n_it_ext++; }
            }
        }
    }
    if (P.wave_clock && lane == 0)
        P.wave_clock[3 * ((size_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) + 1] = __builtin_amdgcn_s_memrealtime();
    if (STATS) {
        const uint64_t a = wave_sum((uint64_t)cn.nodes), b = wave_sum((uint64_t)cn.tris);
        const uint64_t c = wave_sum((uint64_t)cn.ext), e = wave_sum((uint64_t)cn.shadow);
        uint64_t wv[7] = {c_refill, c_trav, c_shade, n_iter, n_active, w_inner, w_leaf};
        for (int k = 0; k < 7; ++k) wv[k] = wave_sum(wv[k]);
        if (lane == 0) {
            atomicAdd(P.stats + PRT_DIAG_NODES, (unsigned long long)a);
            atomicAdd(P.stats + PRT_DIAG_TRIS, (unsigned long long)b);
            atomicAdd(P.stats + PRT_DIAG_EXT, (unsigned long long)c);
            atomicAdd(P.stats + PRT_DIAG_SHADOW, (unsigned long long)e);
            // PRT_DIAG_CLK_REFILL .. PRT_DIAG_WAVE_LEAF, in wv's order
            for (int k = 0; k < 7; ++k) atomicAdd(P.stats + PRT_DIAG_CLK_REFILL + k, (unsigned long long)wv[k]);
        }
        uint64_t ph[PRT_DIAG_PHASE_WORDS] = {c_it_ext, c_it_sh, n_it_ext, n_it_sh, lanes_sh};
        for (int k = 0; k < PRT_DIAG_PHASE_WORDS; ++k) ph[k] = wave_sum(ph[k]);
        if (lane == 0)
            for (int k = 0; k < PRT_DIAG_PHASE_WORDS; ++k)
                atomicAdd(P.stats + PRT_DIAG_PHASE + k, (unsigned long long)ph[k]);
        const uint32_t m = wave_max(cn.max_sp);
        if (lane == 0) atomicMax(P.stats + PRT_DIAG_MAX_STACK, (unsigned long long)m);
        const uint32_t nf = wave_sum(cn.nonfinite);
        if (lane == 0 && nf) atomicAdd(P.stats + PRT_DIAG_NONFINITE, (unsigned long long)nf);
        const uint32_t mq = wave_max(cn.max_q);
        if (lane == 0) atomicMax(P.stats + PRT_DIAG_MAX_QUERY, (unsigned long long)mq);
        const uint32_t wt = wave_sum(cn.w_tri);
        if (lane == 0 && wt) atomicAdd(P.stats + PRT_DIAG_WAVE_TRI, (unsigned long long)wt);
        const uint64_t a2 = wave_sum(l_inner), b2 = wave_sum(l_leaf);
        if (lane == 0) {
            atomicAdd(P.stats + PRT_DIAG_LANE_INNER, (unsigned long long)a2);
            atomicAdd(P.stats + PRT_DIAG_LANE_LEAF, (unsigned long long)b2);
        }
    }
}

}  // namespace
}  // namespace prt

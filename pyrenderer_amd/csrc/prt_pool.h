#pragma once
// prt_pool.h — trace_kernel_pool, the block-pooled shadow-query trace kernel (LDS-resident scenes).
#pragma clang fp contract(off)

#include "prt_shade.h"

namespace prt {
namespace {

// Block-pooled shadow queries (LDS-resident scenes, the reference estimator).
//
// trace_kernel's phase-aligned waves alternate an extension iteration (62.5 of 64 lanes query at
// config 2) with a shadow iteration in which only the ~38 lanes that drew an NEE ray query, and
// those shadow iterations took 43 % of the wave time.  Here the four waves of a block run in
// lockstep phases instead:
//   E: every wave refills its idle lanes and runs one closest-hit extension query per busy lane,
//      then shades it; a lane whose NEE sample needs a visibility test writes the shadow ray
//      (o = p, d = w, t_max = t_at_light) to its slot of the block's LDS pool and its thread id
//      to the block's shadow queue;
//   S: (after a barrier) the queue's n rays are traversed by the first waves to claim them, one per
//      free lane (64 per wave) — whichever wave issued them — and each lane writes the any-hit result to the
//      owner's slot; the other waves are idle (their SIMD slots go to other blocks' waves);
//   R: (after a second barrier) each owner adds its pending NEE radiance if unoccluded and moves
//      on to its next bounce.
// So shadow rays are traversed 64 to a wave instead of ~38, and a lane waits for its shadow
// result without blocking its wave's next extension query.  Before writing a shadow ray, the
// lane tests it against the sampled light triangle itself (one exact Moller-Trumbore test in
// the traversal's arithmetic): the reference's t_at_light bound lets the light occlude itself
// (SURVEY.md §0), and such a ray is answered without a query.  The result of every query is
// unchanged (an any-hit query answers "hit" iff some triangle passes the test, whichever is
// tested first), so images stay bit-identical to trace_kernel's and to the oracle's.
//
// LDS (per 256-thread block): the 16-bit traversal stacks (P.lds_stack entries), the pool (7
// f32 arrays of 256: o.xyz, d.xyz, t_max; t_max carries the result back), the queue (256 u8),
// two parity-alternating control words pairs (queue length, "alive"), then the scene copy:
// octant nodes of the BVH4 or BVH8 (BW), triangles, light triangles and offsets.  Shading data (normals, frames,
// materials) are read from global memory (L1-resident) to keep seven blocks per CU.
// (prt_lds_layout.h pool_lds: the regions' offsets, and kPoolF4, kQueueF4, kCtlF4)
constexpr int kPoolSPrio = 2;                  // issue priority of the S-phase waves (s_setprio)

// One block barrier per iteration (round 4; round 3's kernel had two: after E and after S, with
// the answers resolved in between).  A lane's S answer is resolved in the NEXT iteration, after
// its next extension traversal (which does not depend on it) and before it shades that hit, so
// the reference's order of additions holds and images stay bit-identical.  A wave with a pending
// shadow ray waits only until the previous S phase's entries are answered (an LDS counter, normally
// done by then); S waves run beside the other waves' next traversals, and waves without a claim go
// straight on to their refill (C2 4.049 vs 4.080 ms, C3 at 1024^2 x 32 spp 9.455 vs 9.570 ms per
// launch against the two-barrier kernel, profiles/r04/pool1b/).
// Suspended extension tails (round 7, P.pool_resume_min): a wave's extension traversal lasted as long
// as its longest query (7.4 node and 9.6 triangle trips for queries of 3.2 visits and 3.3 tests).  The
// wave now leaves it once at most pool_resume_min lanes are still traversing; those lanes park their
// traversal state in rows 3..5 of their pool slot, skip shading, keep their item and resume in the next
// iteration, while the finished lanes shade and are refilled.  A suspended lane's LDS stack holds its
// query, so it answers no pooled shadow ray: the S phase hands the queue to the waves' free lanes and
// counts answered entries (every enqueuing lane is free, so the free lanes cover the queue).  Which
// lane finishes when changes no query's result: images stay bit-identical.  C2 3.79 -> 3.61 ms per
// one-frame launch at 12 lanes (profiles/r07/pool_resume/).
// PLAIN: the lean build for scenes without spheres and metal / dielectric materials (P.plain; C1, C2,
// C5): without that code the kernel's loop keeps 17 fewer uniform values in spilled SGPRs and is a
// third shorter
// BW: children per node of the scene's LDS-resident tree (4: the BVH4; 8: the BVH8, visit_node8)
template <bool STATS, int WPE, bool PLAIN, int BW>
__global__ __attribute__((amdgpu_flat_work_group_size(kBlock, kBlock), amdgpu_waves_per_eu(WPE)))
void trace_kernel_pool(TraceParams P) {
    extern __shared__ float4 smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const PoolLds lay = pool_lds(lds_sizes(P, P.lds_stack, BW));   // prt_lds_layout.h
    LdsStack16A stk = LdsStack16A::at(smem, tid);
    using Stk = decltype(stk);
    float* pool = reinterpret_cast<float*>(smem + lay.pool);   // [7][256]
    uint8_t* queue = reinterpret_cast<uint8_t*>(smem + lay.queue);
    uint32_t* ctl = reinterpret_cast<uint32_t*>(smem + lay.ctl);
    float4* sn = smem + lay.nodes;
    float4* st4 = smem + lay.tris;
    float4* slv = smem + lay.light_v;
    int* slo = reinterpret_cast<int*>(smem + lay.light_off);
    float4* smt = smem + lay.mats;   // materials, after the light offsets
    copy_octant_tree<BW>(sn, P.nodes, P.n_node_f4);
    for (int i = tid; i < P.n_tri_f4; i += kBlock) st4[i] = P.tris[i];
    for (int i = tid; i < 4 * P.n_lt; i += kBlock) slv[i] = P.light_v[i];
    for (int i = tid; i <= P.n_light; i += kBlock) slo[i] = P.light_off[i];
    for (int i = tid; i < 2 * P.n_mat; i += kBlock) smt[i] = reinterpret_cast<const float4*>(P.mats)[i];
    if (tid < 4 * kCtlF4) ctl[tid] = 0u;
    __syncthreads();
    const float4* g_nodes = sn;
    const float4* g_tris = st4;
    // normals and shading frames come from global memory (L1-resident): with either the LDS copy
    // no longer fits seven blocks per CU at config 2; the materials sit in LDS (C2 -1.3 %, C3
    // -1.8 % against global loads, profiles/r03/s9/)
    const float4* s_nm = P.tri_nm;
    const float4* s_fr = P.tri_frame;
    const float* s_mats = reinterpret_cast<const float*>(smt);

    uint32_t q_next = 0, q_end = 0;
    bool exhausted = false;
    int item = -1;
    int bounce = 0;
    bool my_sh = false;      // this lane waits for the result of its pooled shadow ray
    // this lane's extension query was suspended (P.pool_resume_min): its traversal state is parked in rows
    // 3..5 of its pool slot and its LDS stack holds the query's entries, so it takes no S work
    bool susp = false;
    uint32_t st = 0;
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0), wi = v3(0, 0, 0);
    V3 beta = v3(1, 1, 1), L = v3(0, 0, 0), pend = v3(0, 0, 0);
    Counters cn = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t n_e = 0, n_s = 0, lanes_s = 0, pre_hits = 0;
    uint64_t n_susp = 0, n_res = 0;   // STATS (PRT_DIAG_SUSPENDED, PRT_DIAG_RESUMED): queries suspended, resumed
    // STATS lane table (PRT_DIAG_LANE_TABLE, tools/lane_table.py): (wave trips, lane trips) of E inner
    // visits, E triangle tests, S inner visits, S triangle tests, the shading block, the Lambert
    // block, the loop iteration (lanes busy after the refill) and the resolve of shadow answers
    uint64_t lt[PRT_DIAG_LANE_TABLE_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // books a traversal's trip counters into lane-table entries k, k + 1 (inner) and k + 2, k + 3 (leaf)
    auto book_trav = [&](int k) {
        lt[k] += cn.wi; lt[k + 1] += cn.li; lt[k + 2] += cn.wl; lt[k + 3] += cn.ll;
        cn.wi = 0; cn.li = 0; cn.wl = 0; cn.ll = 0;
    };
    auto book = [&](int k) {
        uint32_t w = 0, l = 0;
        wave_tick(w, l);
        lt[k] += w; lt[k + 1] += l;
    };
    uint32_t chunk_s = 0, chunk_xy0 = 0;
    // control words (kCtlF4): queue length [0..2], alive [3..5], queue entries claimed [6..8], entries
    // answered [9..11], one triple entry per iteration mod 3 (a slot is reset two iterations after its use)
    uint32_t slot = 0, slot_prev = 0, nq_prev = 0;
    // the queue's buffer (2 x 256 entries) alternates with the iteration's parity: entries enqueued in
    // iteration i are read in i's S phase, and the next enqueue into the
    // same buffer (iteration i + 2) comes after barrier i + 1, which every reader has passed
    uint32_t qpar = 0;
#ifdef PRT_POOL_CLOCKS
    // diagnostic build (tools/pool_clocks.py): wave-level cycles in E, at barrier 1, in S, at barrier 2
    uint64_t ck[PRT_DIAG_POOL_CLOCKS_WORDS] = {0, 0, 0, 0, 0, 0};
    uint64_t t_c = __builtin_amdgcn_s_memtime();
#define PRT_CLOCK(k) do { const uint64_t t_n = __builtin_amdgcn_s_memtime(); ck[k] += t_n - t_c; t_c = t_n; } while (0)
#else
#define PRT_CLOCK(k) do {} while (0)
#endif
    // work-queue refill of the wave's idle lanes (path regeneration; the chunk claim is prt_shade.h
    // claim_chunk; the start of an item is written out as in trace_kernel, see there)
    auto refill = [&](KParams& Q) {
            bool me_idle = item < 0;
            uint64_t idle = __ballot(me_idle);
            for (int round = 0; round < 2 && idle; ++round) {
                uint32_t avail = q_end - q_next;
                if (avail == 0 && !exhausted) {
                    exhausted = !claim_chunk<false, false>(Q, lane, q_next, q_end, chunk_s, chunk_xy0);
                    avail = q_end - q_next;
                }
                if (avail == 0) break;
                uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                uint32_t need = (uint32_t)__popcll(idle);
                uint32_t take = need < avail ? need : avail;
                if (me_idle && rank < take) {
                    item = (int)(q_next + rank);
                    L = v3(0, 0, 0);
                    int x, y;
                    pixel_of(Q, (uint32_t)item, chunk_s, chunk_xy0, x, y);
                    int W = Q.W, H = Q.H;
                    asm volatile("" : "+s"(W), "+s"(H));
                    bool ok = x < W && y < H;
                    if (ok) {
                        // primary rays from camera_kernel (or caller rays): no camera code in the loop —
                        // its uniform operands spilled 36 more SGPRs (C2 4.01 -> 3.91 ms without it)
                        float4 r = Q.rays[item];
                        d = v3(r.x, r.y, r.z);
                        st = __float_as_uint(r.w);
                        if (Q.ray_o) {
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
                        item = -2;
                    } else {
                        beta = v3(1, 1, 1);
                        bounce = 0;
                        // the primary ray as this lane's next ray (R takes o from the pool, d from wi)
                        pool[0 * kBlock + tid] = o.x; pool[1 * kBlock + tid] = o.y; pool[2 * kBlock + tid] = o.z;
                        wi = d;
                    }
                }
                q_next += take;
                me_idle = item == -1;
                idle = __ballot(me_idle);
            }
        if (item == -2) item = -1;
    };
    while (true) {
        // the launch parameters are re-read each iteration through the kernarg pointer (scalar loads from
        // the constant cache): kept live across the loop they exceeded the SGPR budget and were spilled
        // into VGPR lanes, reloaded by v_readlane in every refill
        KParams& Q = kernarg();
        // ------------------------------------------------------------------ E phase
        refill(Q);
        PRT_CLOCK(4);
        if (STATS && item >= 0) book(12);
        // (a) extension traversal: every busy lane except one whose pending shadow ray ends its path
        const bool trav = item >= 0 && !(my_sh && bounce + 1 >= Q.depth);
        // The wave leaves the traversal once at most pool_resume_min lanes are still traversing (RES,
        // traverse_ww4; 0: never, 64: after every round that leaves a lane unfinished): those lanes keep their query (ts, their LDS stack, the same (o, d)) and resume it
        // in the next iteration, the finished ones shade and are refilled.  Off once the work queue is
        // exhausted: suspending pays only while finished lanes can be refilled.
        int hid = -1;
        float ht = 0.0f;
        bool hit = false, done = false;
        TState ts = {0, 0, 0, 0, 0.0f};
        if (__ballot(trav) != 0) {
            if (STATS && lane == __builtin_amdgcn_readfirstlane(lane)) n_e++;
            if (trav) {
                if (susp) {
                    const uint32_t cl = __float_as_uint(pool[3 * kBlock + tid]), sb = __float_as_uint(pool[4 * kBlock + tid]);
                    ts.cur = (int)(short)(cl & 0xFFFFu); ts.leaf = (int)cl >> 16;
                    ts.sp = (int)(sb & 0xFFFFu); ts.best_id = (int)sb >> 16;
                    ts.best = pool[5 * kBlock + tid];
                    if (STATS) n_res++;
                } else {
                    tstate_init(ts, stk, kTMax);
                    if (STATS) { cn.ext++; cn.q0 = cn.nodes; }
                }
                done = traverse_ww4<STATS, 1, Stk, false, true, true, BW>(
                    g_nodes, g_tris, o, d, kTMin, kTMax, false, stk, hid, ht, cn, &ts, exhausted ? 0 : Q.pool_resume_min + 1,
                    Q.fault, exhausted ? 0 : Q.leaf_break, exhausted ? 0 : Q.leaf_exit, Q.guard_trips);
                hit = done && hid >= 0;
                if (STATS) {
                    if (done) cn.max_q = max(cn.max_q, cn.nodes - cn.q0);
                    book_trav(0);
                }
                // spheres once, against the completed query's closest triangle
                if (!PLAIN && done && Q.n_sph > 0) {
                    float best = hit ? ht : kTMax;
                    for (int k = 0; k < Q.n_sph; ++k) {
                        float root;
                        if (sphere_hit(Q.sph[k], o, d, kTMin, best, root)) {
                            best = root;
                            hid = Q.n_tri + k;
                            hit = true;
                        }
                    }
                    ht = best;
                }
            }
        }
        PRT_CLOCK(5);
        // (b) the previous S phase's answers (its waves ran it beside this wave's traversal): a wave
        // with a pending shadow ray waits until every entry of the previous queue has been answered
        if (__ballot(my_sh) != 0) {
            // bounded: a wait that never ends (a logic error) raises the watchdog flag instead of
            // hanging the device: 2^20 sleeps of 64 clocks ~ 30 ms, against a worst case of ~0.1 ms for
            // the answers (an LDS scene is <= 24 KiB: a query visits each of its <= ~100 nodes and
            // <= ~500 triangles at most once, ~10^5 cycles even in a STATS build).  A lane whose answer
            // did not arrive ends with NaN radiance (counted by STATS' non-finite samples), so a tripped
            // wait cannot pass for a valid image even before prt_check_faults reports it.
            bool late = false;
            const uint32_t need = nq_prev;
            for (uint32_t spin = 0;
                 need && __hip_atomic_load(&ctl[9 + slot_prev], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need;
                 ++spin) {
                if (spin >= (1u << 20)) {
                    if (lane == 0) atomicOr(Q.fault, 2);
                    late = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (my_sh) {
                if (STATS) book(14);
                const float r = pool[6 * kBlock + tid];
                if (late) L = v3(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000));
                else if (r == r) L = L + pend;   // not occluded
                my_sh = false;
                ++bounce;
                if (bounce >= Q.depth) finish_sample<STATS>(Q, item, L, cn);
            }
        }
        // A suspended query parks its state in rows 3..5 of its lane's pool slot (free after (b): the lane
        // enqueues no shadow ray, and the previous S phase has read the one it had), so the state holds no
        // registers across shading and the S phase: cur | leaf << 16, sp | best_id << 16 (16-bit references
        // and LDS addresses, lds_fits4), best.  The lane skips (c) and keeps its item.
        susp = trav && !done;
        if (susp) {
            pool[3 * kBlock + tid] = __uint_as_float(((uint32_t)ts.cur & 0xFFFFu) | ((uint32_t)ts.leaf << 16));
            pool[4 * kBlock + tid] = __uint_as_float(((uint32_t)ts.sp & 0xFFFFu) | ((uint32_t)ts.best_id << 16));
            pool[5 * kBlock + tid] = ts.best;
            if (STATS) n_susp++;
        }
        // (c) shading of this iteration's completed extension queries
        if (trav && done) {
            if (STATS) book(8);
            {
                bool finished = false;
                if (!hit) {
                    finished = true;
                } else {
                    const Surface sf = hit_surface<PLAIN>(Q, s_nm, s_mats, o, d, ht, hid);
                    const V3 p = sf.p, ng = sf.ng, n = sf.n;
                    const float* m = sf.m;
                    const bool flip = sf.flip;
                    if (!PLAIN && (m[5] == 2.0f || m[5] == 3.0f)) {
                        bool absorbed;
                        const V3 out = specular_scatter(m, d, ng, st, absorbed);
                        if (absorbed) {
                            finished = true;
                        } else {
                            beta = beta * v3(m[0], m[1], m[2]);
                            wi = normalize(out);   // next ray (p, wi), taken up in R
                            ++bounce;
                            if (bounce >= Q.depth) finished = true;
                        }
                    } else if (m[3] != 0.0f) {
                        float d1 = dot(neg(d), n);
                        if (d1 > 0.0f) {
                            V3 lc = v3(Q.dl_r, Q.dl_g, Q.dl_b);
                            L = bounce == 0 ? L + lc * beta : L + (lc * beta) * d1;
                        }
                        finished = true;
                    } else {
                        if (STATS) book(10);
                        // lambert_dir's text, written out: through the shared function config 3 ran 0.2 % slower
                        // per launch (profiles/r08/shared_shading/ab_c3_lambert_dir.jsonl)
                        float u0 = rng_next(st);
                        float u1 = rng_next(st);
                        V3 l = cosine_hemisphere<true>(u0, u1);
                        const float4* fr = s_fr + ((size_t)((PLAIN || hid < Q.n_tri) ? hid : 0) * 2 + (flip ? 1 : 0)) * 3;
                        if (PLAIN || hid < Q.n_tri) {
                            float4 f0 = fr[0], f1 = fr[1], f2 = fr[2];
                            wi = normalize<true>(xyz(f0) * l.x + xyz(f1) * l.y + xyz(f2) * l.z);
                        } else {
                            wi = to_world(n, l);
                        }
                        beta = beta * lambert_weight<true>(m, n, wi, Q.shade_fast);
                        const LightSample ls = sample_light<true>(Q, slo, slv, st);
                        const float4 L0 = ls.v0, L1 = ls.v1, L2 = ls.v2, LN = ls.nm;
                        const V3 p2 = ls.p2, n2 = xyz(LN);
                        const NeeRay nr = nee_ray<true>(p, n, p2, n2);
                        const V3 w = nr.w;
                        const float t_at = nr.t_at, dot1 = nr.dot1, dot2 = nr.dot2;
                        bool queued = false;
                        if (dot1 > 0.0f && dot2 > 0.0f) {
                            if (STATS) cn.shadow++;
                            // the sampled light triangle itself, in the traversal's arithmetic: a hit
                            // in (t_min, t_at_light) answers the any-hit query (occluded)
                            float tl;
                            const V3 lv0 = xyz(L0);
                            const bool self_hit = mt_u(lv0, xyz(L1) - lv0, xyz(L2) - lv0, p, w, kTMin, t_at, 0, -1,
                                                       true, tl);
                            if (STATS) { cn.tris++; pre_hits += self_hit ? 1 : 0; }
                            if (!self_hit) {
                                const float* em = s_mats + 8 * __float_as_int(LN.w);
                                pend = beta * nee_radiance<true>(em, p, p2, dot1, dot2, Q.shade_fast);
                                pool[3 * kBlock + tid] = w.x; pool[4 * kBlock + tid] = w.y; pool[5 * kBlock + tid] = w.z;
                                pool[6 * kBlock + tid] = t_at;
                                queued = true;
                            }
                        }
                        if (queued) {
                            my_sh = true;
                        } else {
                            ++bounce;
                            if (bounce >= Q.depth) finished = true;
                        }
                    }
                    // every continuing lane parks its next ray's origin p in its pool slot (the
                    // shadow ray's origin too) and its direction in wi: neither stays live in
                    // registers across the S phase, where the lane may traverse another lane's ray
                    pool[0 * kBlock + tid] = p.x; pool[1 * kBlock + tid] = p.y; pool[2 * kBlock + tid] = p.z;
                }
                if (finished) finish_sample<STATS>(Q, item, L, cn);
            }
        }
        // enqueue this wave's shadow rays: one LDS atomic per wave, thread ids at the ranks
        {
            const uint64_t m = __ballot(my_sh);
            const uint32_t cnt = (uint32_t)__popcll(m);
            uint32_t base = 0;
            if (cnt) {
                if (lane == __builtin_amdgcn_readfirstlane(lane)) base = atomicAdd(&ctl[slot], cnt);
                base = __builtin_amdgcn_readfirstlane(base);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (my_sh) queue[qpar * kBlock + base + rank] = (uint8_t)tid;
            }
            // a wave with busy lanes or unclaimed work keeps the block looping
            if ((__ballot(item >= 0) != 0 || !exhausted) && lane == 0) ctl[3 + slot] = 1u;
            // the next iteration's words, last used two iterations ago (every wave has read them since)
            if (tid == 0) {
                const uint32_t ns = slot == 2 ? 0u : slot + 1u;
                ctl[ns] = 0u; ctl[3 + ns] = 0u; ctl[6 + ns] = 0u; ctl[9 + ns] = 0u;
            }
        }
        PRT_CLOCK(0);
        __syncthreads();
        PRT_CLOCK(1);
        // ------------------------------------------------------------------ S phase
        const uint32_t n_q = ctl[slot];
        // the queue's rays go to the free lanes (those holding no suspended query: an S traversal uses
        // the lane's own stack) of the first waves to claim some, one claim per wave of as many
        // entries as it has free lanes; the others refill the lanes that finished in E meanwhile, off
        // the critical path.  Every enqueuing lane is free, so the block's free lanes cover the queue.
        // Without suspended lanes these are the 64-ray chunks of the earlier kernel and one partial
        // (equal-size chunks: C2 +0.5 %, C3 +0.8 %; the arrival-ordered claim with an early refill by
        // the first two waves at barrier 1: C2 +1.2 %, C3 +0.9 %; profiles/r03/pool/)
        const uint64_t free_m = __ballot(!susp);
        const uint32_t n_free = (uint32_t)__popcll(free_m);
        uint32_t e0 = 0xFFFFFFFFu;
        if (n_q && n_free) {
            if (lane == 0) e0 = atomicAdd(&ctl[6 + slot], n_free);
            e0 = __builtin_amdgcn_readfirstlane(e0);
        }
        if (e0 < n_q) {
            // the S waves hold up their whole block at barrier 2: issue priority over other blocks
            __builtin_amdgcn_s_setprio(kPoolSPrio);
            const uint32_t e1 = min(n_q, e0 + n_free);
            const uint32_t e = e0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(free_m >> 32),
                                                             __builtin_amdgcn_mbcnt_lo((uint32_t)free_m, 0u));
            if (STATS && lane == 0) { n_s++; lanes_s += e1 - e0; }
            const bool sq = !susp && e < e1;
            int owner = 0;
            V3 so = v3(0, 0, 0), sd = v3(1, 1, 1);
            float stm = 0.0f;
            if (sq) {
                owner = queue[qpar * kBlock + e];
                so = v3(pool[0 * kBlock + owner], pool[1 * kBlock + owner], pool[2 * kBlock + owner]);
                sd = v3(pool[3 * kBlock + owner], pool[4 * kBlock + owner], pool[5 * kBlock + owner]);
                stm = pool[6 * kBlock + owner];
            }
            if (sq) {
                int hid = -1;
                float ht = 0.0f;
                if (STATS) cn.q0 = cn.nodes;
                bool hit = traverse_ww4<STATS, 2, Stk, false, false, true, BW>(
                    g_nodes, g_tris, so, sd, kTMin, stm, true, stk, hid, ht, cn, nullptr, 0, Q.fault,
                    exhausted ? 0 : Q.leaf_break, exhausted ? 0 : Q.leaf_exit, Q.guard_trips);
                if (STATS) { cn.max_q = max(cn.max_q, cn.nodes - cn.q0); book_trav(4); }
                if (!PLAIN) sphere_hits(Q, so, sd, kTMin, stm, true, hit, hid, ht);
                // the result travels back in the owner's t_max word: NaN = occluded
                pool[6 * kBlock + owner] = hit ? __int_as_float(0x7FC00000) : 0.0f;
            }
            __builtin_amdgcn_s_setprio(0);
            // publish the answers (LDS stores above) before counting the entries as answered
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_fetch_add(&ctl[9 + slot], e1 - e0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        nq_prev = n_q;
        PRT_CLOCK(2);
        const bool alive = ctl[3 + slot] != 0u;
        slot_prev = slot;
        slot = slot == 2 ? 0u : slot + 1u;
        qpar ^= 1u;
        // the next extension ray: origin from the pool slot, direction wi (no register keeps the
        // previous ray across the S phase, where the lane may traverse another lane's ray)
        o = v3(pool[0 * kBlock + tid], pool[1 * kBlock + tid], pool[2 * kBlock + tid]);
        d = wi;
        if (!alive) break;
    }
#ifdef PRT_POOL_CLOCKS
    if (lane == 0)
        for (int k = 0; k < PRT_DIAG_POOL_CLOCKS_WORDS; ++k)
            atomicAdd(P.stats + PRT_DIAG_POOL_CLOCKS + k, (unsigned long long)ck[k]);
#endif
#undef PRT_CLOCK
    if (STATS) {
        // the four counters (PRT_DIAG_NODES ..), then the pooled kernel's PRT_DIAG_POOL words
        const uint64_t sums[4 + PRT_DIAG_POOL_WORDS] = {cn.nodes, cn.tris, cn.ext,  cn.shadow,
                                                        n_e,      n_s,     lanes_s, pre_hits};
        for (int k = 0; k < 4 + PRT_DIAG_POOL_WORDS; ++k) {
            const uint64_t v = wave_sum(sums[k]);
            const int word = k < 4 ? PRT_DIAG_NODES + k : PRT_DIAG_POOL + k - 4;
            if (lane == 0) atomicAdd(P.stats + word, (unsigned long long)v);
        }
        for (int k = 0; k < PRT_DIAG_LANE_TABLE_WORDS; ++k) {
            const uint64_t v = wave_sum(lt[k]);
            if (lane == 0 && v) atomicAdd(P.stats + PRT_DIAG_LANE_TABLE + k, (unsigned long long)v);
        }
        n_susp = wave_sum(n_susp);
        n_res = wave_sum(n_res);
        if (lane == 0 && n_susp) {
            atomicAdd(P.stats + PRT_DIAG_SUSPENDED, (unsigned long long)n_susp);
            atomicAdd(P.stats + PRT_DIAG_RESUMED, (unsigned long long)n_res);
        }
        const uint32_t msp = wave_max(cn.max_sp), nf = wave_sum(cn.nonfinite), mq = wave_max(cn.max_q);
        if (lane == 0) {
            atomicMax(P.stats + PRT_DIAG_MAX_STACK, (unsigned long long)msp);
            if (nf) atomicAdd(P.stats + PRT_DIAG_NONFINITE, (unsigned long long)nf);
            atomicMax(P.stats + PRT_DIAG_MAX_QUERY, (unsigned long long)mq);
        }
    }
}

}  // namespace
}  // namespace prt

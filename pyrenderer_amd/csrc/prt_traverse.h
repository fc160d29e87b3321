#pragma once
// prt_traverse.h — the per-lane traversal stacks and the while-while traversal (traverse_ww4) of the BVH4
// in its three forms and of the LDS-resident scenes' BVH8.
#pragma clang fp contract(off)

#include "prt_math.h"

namespace prt {
namespace {

// ---------------------------------------------------------------- traversal
struct Counters {
    uint32_t nodes, tris, ext, shadow, it_inner, it_leaf, max_sp, nonfinite, w_tri, q0, max_q;
    // STATS lane table (trace_kernel_pool, diag words 160..): wave-level trips of the traversal's
    // inner-node and triangle loops, and the active lanes summed over those trips (wave_tick)
    uint32_t wi, li, wl, ll;
};
// STATS: one wave-level trip of the enclosing loop body, booked by its first active lane, with
// the lanes active in it: sum(l) / (64 sum(w)) is that loop's SIMD lane utilisation
__device__ __forceinline__ void wave_tick(uint32_t& w, uint32_t& l) {
    const uint32_t pc = (uint32_t)__popcll(__ballot(true));
    if ((uint32_t)__builtin_amdgcn_readfirstlane(__lane_id()) == __lane_id()) { w += 1u; l += pc; }
}

// Moller-Trumbore in the reference's exact expression order
// (intersection_taichi.py:69-91), for closest-hit and any-hit lanes of one wave.
// nodes/tris point either to global memory or to the block's LDS copy of a
// small scene (the compiler infers the address space after inlining).
__device__ __forceinline__ bool mt_u(V3 v0, V3 e1, V3 e2, V3 o, V3 d, float t0, float tbest, int id, int best_id,
                                     bool any, float& tout) {
    // branch-free: a lane failing an early test would wait for the wave's other lanes
    // anyway, so every value is computed and the tests are combined (same results as the
    // reference's early returns; det == 0 is rejected, its quotient never used)
    V3 c = cross(e1, d);
    float det = dot(c, e2);
    const bool nz = fabsf(det) > 0.0f;
    float f = rcp_exact(det);   // det == 0 takes rcp_exact's division (inf): masked by nz below
    V3 s = o - v0;
    V3 q = cross(s, e2);
    float t = -f * dot(q, e1);
    float u = -f * dot(q, d);
    float v = f * dot(c, s);
    // bitwise (not short-circuit) combination: one lane mask, no exec-mask branches
    const bool in_range = (t0 < t) & ((t < tbest) | ((!any) & (t == tbest) & (id < best_id)));
    const bool hit = nz & in_range & (0.0f <= u) & (u <= 1.0f) & (v >= 0.0f) & (1.0f - u - v >= 0.0f);
    tout = t;
    return hit;
}

// While-while traversal (Aila & Laine 2009, "persistent while-while"): lanes
// descend inner nodes until every lane of the wave holds a postponed leaf,
// then all lanes test leaf triangles together, so inner-node and leaf work
// of different lanes do not serialise against each other.  Stack bottom
// holds kSentinel; leaves are negative references, inner nodes >= 0.
constexpr int kSentinel = 0x7FFFFFFF;
constexpr uint32_t kGuardTrips = 1u << 20;   // leaf batches per query before the watchdog trips

// While-while over the BVH4 (prt_internal.h): one node fetch tests four child
// boxes; the nearest hit child is visited next (a 3-comparator tournament) and the
// other hit children are pushed.

// Per-lane traversal stacks.  LdsStack: entry k at l[k * kBlock] (conflict-free).
// SpillStack: the first LST entries in LDS, deeper ones in a per-lane global area
// (stride = all threads of the grid); deep stacks are rare (max 24 entries measured on
// the 1 M-triangle scene against a worst-case bound of 46), so a small LDS stack keeps
// occupancy and the spill branch is almost never taken.
struct LdsStack {
    static constexpr int kSent = kSentinel;
    static constexpr int kStep = 1;   // sp advances by kStep per entry (LdsStack16A: bytes)
    int* l;
    __device__ __forceinline__ int origin() const { return 0; }
    __device__ __forceinline__ int depth(int sp) const { return sp; }
    __device__ __forceinline__ void put(int k, int v) { l[k * kBlock] = v; }
    __device__ __forceinline__ int get(int k) const { return l[k * kBlock]; }
    // entries [0, k] of every lane are in LDS (always)
    __device__ __forceinline__ bool lds_only(int) const { return true; }
    __device__ __forceinline__ LdsStack lds() const { return *this; }
};
template <int LST>
struct SpillStack {
    static constexpr int kSent = kSentinel;
    static constexpr int kStep = 1;
    int* l;
    __device__ __forceinline__ int origin() const { return 0; }
    __device__ __forceinline__ int depth(int sp) const { return sp; }
    int* g;
    uint32_t gs;
    __device__ __forceinline__ void put(int k, int v) {
        if (k < LST) l[k * kBlock] = v;
        else g[(size_t)(k - LST) * gs] = v;
    }
    __device__ __forceinline__ int get(int k) const { return k < LST ? l[k * kBlock] : g[(size_t)(k - LST) * gs]; }
    // wave-uniform: no lane touches an entry above k < LST, so the spill branches can go
    __device__ __forceinline__ bool lds_only(int k) const { return __ballot(k >= LST) == 0; }
    __device__ __forceinline__ LdsStack lds() const { return LdsStack{l}; }
};
// LDS-resident scenes: 16-bit entries (half the stack's LDS, so the octant node copies
// fit beside it at six blocks per CU).  Node indices and leaf references of such scenes fit
// 16 bits (host check in lds_fits4), and the traversal sentinel is 0x7FFF: the block's LDS
// copy of the BVH4 rewrites the empty-slot references to it.  Entry k of lane j sits at
// 2 * (k * kBlock + (j & ~63) + 2 * (j & 31) + (j >> 5 & 1)): a half-wave's 32 lanes use 32
// different banks.
constexpr int kSentinel16 = 0x7FFF;
// The stack pointer is held as the entry's LDS byte ADDRESS (round 6): a push writes at
// sp + kStep as an immediate offset of the pointer register and advances it by a select, a pop reads at
// sp — no per-entry address arithmetic (the index form spends a v_lshl_add on every push and pop:
// three or four per node visit; C2 -0.2 %, C3 -0.5 % per launch against it, profiles/r06/stack/)
typedef __attribute__((address_space(3))) short LdsShort;
struct LdsStack16A {
    static constexpr int kSent = kSentinel16;
    static constexpr int kStep = 2 * kBlock;
    int base;   // LDS byte address of this lane's entry 0
    __device__ __forceinline__ void put(int k, int v) { *(LdsShort*)(uintptr_t)(uint32_t)k = (short)v; }
    __device__ __forceinline__ int get(int k) const { return (int)*(const LdsShort*)(uintptr_t)(uint32_t)k; }
    __device__ __forceinline__ int origin() const { return base; }
    __device__ __forceinline__ int depth(int sp) const { return (sp - base) / kStep; }
    __device__ __forceinline__ bool lds_only(int) const { return true; }
    __device__ __forceinline__ LdsStack16A lds() const { return *this; }
    // lane t's stack in the block's stack area at `smem`
    static __device__ __forceinline__ LdsStack16A at(const void* smem, int t) {
        return LdsStack16A{(int)(uintptr_t)(LdsShort*)((short*)smem + (t & ~63) + 2 * (t & 31) + ((t >> 5) & 1))};
    }
};
// sp advanced by one entry where p holds.  Address form: the 0 / 1 select laundered into a register and
// shifted by the entry stride (one v_cndmask + one v_lshl_add); as a select of 0 / 512 the stride would
// need a VGPR of its own (gfx950 reads one scalar operand per VALU instruction besides the mask), which
// the pooled kernel pays with spills
template <class S>
__device__ __forceinline__ int stack_adv(int sp, bool p) {
    if constexpr (S::kStep == 1) {
        return sp + (p ? 1 : 0);
    } else {
        int b = p ? 1 : 0;
        asm volatile("" : "+v"(b));
        return sp + (b << __builtin_ctz(S::kStep));
    }
}

// LDS-resident scene data (the block's octant node copies and triangles) addressed as LDS: the
// element offset stays a 32-bit LDS address (v_mad_u32_u24 / v_lshl_add) instead of the 64-bit
// flat-pointer arithmetic (v_mad_u64_u32) the generic pointer gets before address-space inference
// (measured against the flat form: C2 3.878 vs 3.890 ms, C3 70.97 vs 71.26 ms per launch, profiles/r05/micro/)
typedef float F4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const F4v LdsF4;
__device__ __forceinline__ const LdsF4* as_lds(const float4* p) { return (const LdsF4*)p; }
// one ds_read_b128 of element i
__device__ __forceinline__ float4 lds4(const LdsF4* p, int i) {
    const F4v v = p[i];
    return make_float4(v.x, v.y, v.z, v.w);
}

// Slab test from plane distances already ordered near/far (quantised nodes).
__device__ __forceinline__ bool slab_t(float nx, float fx, float ny, float fy, float nz, float fz, float tmin,
                                       float tmax, float& tn) {
    float tnear = fmaxf(fmaxf(nx, ny), fmaxf(nz, tmin));
    float tfar = fminf(fminf(fx, fy), fminf(fz, tmax)) * kGamma;
    tn = tnear;
    return tnear <= tfar;
}
__device__ __forceinline__ float ubyte(uint32_t w, int k) {
    return (float)((w >> (8 * k)) & 0xFFu);   // v_cvt_f32_ubyte{k}
}
// Child k of a quantised node (prt_internal.h): plane distance (origin + q s - o) / d
// evaluated as fma(q, s/d, (origin - o)/d); the >= 2 pad outward rounding of the grid
// covers the estimate's error, so the test stays conservative.  The q words arrive
// already swapped into near/far order by the sign of 1/d (see slab_nf()).
struct QAxis { float A, B; };
__device__ __forceinline__ bool qchild(int k, uint32_t lxq, uint32_t hxq, uint32_t lyq, uint32_t hyq, uint32_t lzq,
                                       uint32_t hzq, QAxis X, QAxis Y, QAxis Z, float tmin, float tmax, float& tn) {
    return slab_t(__builtin_fmaf(ubyte(lxq, k), X.A, X.B), __builtin_fmaf(ubyte(hxq, k), X.A, X.B),
                  __builtin_fmaf(ubyte(lyq, k), Y.A, Y.B), __builtin_fmaf(ubyte(hyq, k), Y.A, Y.B),
                  __builtin_fmaf(ubyte(lzq, k), Z.A, Z.B), __builtin_fmaf(ubyte(hzq, k), Z.A, Z.B), tmin, tmax, tn);
}

// Traversal state of a query that may be suspended between loop iterations (RES).
struct TState { int cur, leaf, sp, best_id; float best; };
// A query whose t_max is NaN (the reference's shadow bound t_at_light = (p2.x - p.x) / w.x
// is 0/0 when p2.x == p.x, core/tracing.py:97) can never accept a triangle: Moller-Trumbore
// needs t < t_max (intersection_taichi.py:84), false against NaN.  Its slab tests never cull
// either (fminf drops the NaN), so traversing would walk every box along the whole line
// (config 4: ~2000 node visits, the launch's last 2 ms); it starts finished instead, with
// the same (miss) result.  Spheres still see the NaN bound (hit_sphere accepts it).
template <class S>
__device__ __forceinline__ int root_for(float tmax) { return tmax == tmax ? 0 : S::kSent; }

template <class S>
__device__ __forceinline__ void tstate_init(TState& ts, S stk, float tmax) {
    stk.put(stk.origin(), S::kSent);
    ts.cur = root_for<S>(tmax); ts.leaf = 0; ts.sp = stk.origin(); ts.best_id = -1; ts.best = tmax;
}

// RES: the wave leaves the traversal loop once fewer than `min_lanes` lanes are still
// traversing; the unfinished lanes keep their state (registers + LDS stack) and resume
// in the next iteration, so the long tail of a few slow lanes no longer idles the
// others.  Returns whether the query finished (hit_id / hit_t valid).
// Conservative slab test on a padded box (PBRT-style 1+2*gamma3 on t_far).
// t = (lo - o) / d is evaluated as fma(lo, 1/d, -o/d): pruning only, so the few-ulp
// error of the estimate is covered by the box padding (~1e-6 of the scene scale,
// >> |o/d| ulp) and the 1+2*gamma3 factor on t_far.  The near and far plane of each
// axis are chosen by the sign of 1/d, NOT by min/max of the two distances: for a
// direction component of exactly 0 (1/d = inf) a plane distance can be NaN, and
// fminf/fmaxf would then turn the other plane's -inf into the FAR distance and cull
// a box the ray lies inside (measured: 8 of 262144 pixels at config 2).  With the
// selection, a NaN distance is dropped by the fmaxf/fminf that follow, which can
// only enlarge the interval.  For f32 BVH4 nodes the selection is an address offset
// (no per-plane selects); quantised nodes swap their plane words (qchild).
__device__ __forceinline__ bool slab_nf(float nx, float fx, float ny, float fy, float nz, float fz, V3 oi, V3 inv,
                                        float tmin, float tmax, float& tn) {
    float ax = __builtin_fmaf(nx, inv.x, -oi.x), bx = __builtin_fmaf(fx, inv.x, -oi.x);
    float ay = __builtin_fmaf(ny, inv.y, -oi.y), by = __builtin_fmaf(fy, inv.y, -oi.y);
    float az = __builtin_fmaf(nz, inv.z, -oi.z), bz = __builtin_fmaf(fz, inv.z, -oi.z);
    float tnear = fmaxf(fmaxf(ax, ay), fmaxf(az, tmin));
    // the reference's 1 + 2 gamma_3 factor on t_far (bvh_taichi.py:179).  The box padding (1e-6 of
    // the scene's largest coordinate, ~8 ulps) alone would keep the test conservative, and dropping the
    // factor saves 4 VALU per visit (measured without it: C2 3.873 vs 3.884, C3 70.75 vs 71.14 ms per
    // launch, images identical), but the pooled kernel then spills 3 VGPRs and writes 0.14 GB more
    // per frame to HBM (profiles/r05/gamma/): kept
    // (fminf canonicalises the loop-carried tmax, one VALU per visit; an asm v_min_f32 without it pins
    // registers: 7 spilled VGPRs, C2 +0.6 %, profiles/r06/guards/)
    float tfar = fminf(fminf(bx, by), fminf(bz, tmax)) * kGamma;
    tn = tnear;
    return tnear <= tfar;
}

// Slab reciprocals 1/d, clamped to +-1e30.  A direction component of exactly +-0 (one cosine
// draw in 2^24) would give 1/d = +-inf, and fma(plane, 1/d, -o/d) = inf - inf = NaN: the
// near/far selection then drops that axis and the ray culls nothing along it, walking every
// box it overlaps in the other two axes (config 4: 1000-2200 node visits for such a query,
// against 25 on average, each one of the launch's slowest paths).  With the clamp the
// distances are +-1e30 (plane - o) up to the rounding of o * 1e30 (|o| 2^-24 1e30), which the
// box padding (>= 1e-6 |o|) covers: the sign is right and the test stays conservative.
__device__ __forceinline__ V3 ray_inv(V3 d) {
    auto c = [](float x) { return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(x), -1e30f, 1e30f); };
    return v3(c(d.x), c(d.y), c(d.z));
}

// One inner-node visit of the while-while BVH4 traversal: tests the four child boxes of
// node `cur`, continues with the nearest hit child (MODE 2, any-hit: the last hit child,
// no sorting) and pushes the other hit children; pops the stack when none is hit.
// Pushes write the slot above the top unconditionally and advance the stack pointer by
// the hit predicate (no exec-mask branches); the highest slot written is the same as
// with conditional pushes (<= 3 above the entry top).
// OCT (LDS-resident scenes): `nodes` is the block's octant copy of the BVH4 (8 copies of each
// node, copy k with the near and far planes of each axis pre-arranged for the direction signs
// k = sx | sy << 1 | sz << 2: 7 float4 = nx, fx, ny, fy, nz, fz, refs; node stride 56 float4)
// and `sx` holds the query's copy offset 7 k: the seven reads need no per-plane addresses.
// Copy k also stores the four children in k's front-to-back order, so closest-hit visits of
// an octant copy take the first hit child instead of sorting entry distances (see step).
template <bool STATS, int MODE, class S, bool QN, bool OCT = false>
__device__ __forceinline__ void visit_node4(const float4* __restrict__ nodes, int& cur, int& sp, S stk, V3 inv, V3 oi,
                                            int sx, int sy, int sz, float tmin, float best, Counters& cn,
                                            bool any_lane = false) {
    float t0, t1, t2, t3;
    bool h0, h1, h2, h3;
    int r0, r1, r2, r3;
    if (QN) {
        // 64-B nodes at a 32-bit byte offset from the uniform base (saddr + voffset addressing,
        // no 64-bit address arithmetic): BVH4 nodes < refs / 3 < 2^25, so the offset < 2^31
        const float4* nd = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(nodes) + ((uint32_t)cur << 6));
        float4 a = nd[0], b = nd[1], c = nd[2], rf = nd[3];
        if (STATS) { cn.nodes++; cn.it_inner++; }
        QAxis X = {a.w * inv.x, __builtin_fmaf(a.x, inv.x, -oi.x)};
        QAxis Y = {b.x * inv.y, __builtin_fmaf(a.y, inv.y, -oi.y)};
        QAxis Z = {b.y * inv.z, __builtin_fmaf(a.z, inv.z, -oi.z)};
        uint32_t lxq = __float_as_uint(sx ? b.w : b.z), hxq = __float_as_uint(sx ? b.z : b.w);
        uint32_t lyq = __float_as_uint(sy ? c.y : c.x), hyq = __float_as_uint(sy ? c.x : c.y);
        uint32_t lzq = __float_as_uint(sz ? c.w : c.z), hzq = __float_as_uint(sz ? c.z : c.w);
        r0 = __float_as_int(rf.x); r1 = __float_as_int(rf.y); r2 = __float_as_int(rf.z); r3 = __float_as_int(rf.w);
        h0 = qchild(0, lxq, hxq, lyq, hyq, lzq, hzq, X, Y, Z, tmin, best, t0) && r0 != kSentinel;
        h1 = qchild(1, lxq, hxq, lyq, hyq, lzq, hzq, X, Y, Z, tmin, best, t1) && r1 != kSentinel;
        h2 = qchild(2, lxq, hxq, lyq, hyq, lzq, hzq, X, Y, Z, tmin, best, t2) && r2 != kSentinel;
        h3 = qchild(3, lxq, hxq, lyq, hyq, lzq, hzq, X, Y, Z, tmin, best, t3) && r3 != kSentinel;
    } else {
        float4 nx, fx, ny, fy, nz, fz, rf;
        if (OCT) {
            const LdsF4* nl = as_lds(nodes) + (int)(__umul24((uint32_t)cur, 56u) + (uint32_t)sx);
            auto nd = [&](int i) { return lds4(nl, i); };
            nx = nd(0); fx = nd(1); ny = nd(2); fy = nd(3); nz = nd(4); fz = nd(5); rf = nd(6);
        } else {
            // near/far planes picked by address (the node stores lo and hi per axis)
            const float4* nd = nodes + (size_t)cur * 8;
            nx = nd[sx]; fx = nd[1 - sx]; ny = nd[2 + sy]; fy = nd[3 - sy]; nz = nd[4 + sz]; fz = nd[5 - sz];
            rf = nd[6];
        }
        if (STATS) { cn.nodes++; cn.it_inner++; }
        h0 = slab_nf(nx.x, fx.x, ny.x, fy.x, nz.x, fz.x, oi, inv, tmin, best, t0);
        h1 = slab_nf(nx.y, fx.y, ny.y, fy.y, nz.y, fz.y, oi, inv, tmin, best, t1);
        h2 = slab_nf(nx.z, fx.z, ny.z, fy.z, nz.z, fz.z, oi, inv, tmin, best, t2);
        h3 = slab_nf(nx.w, fx.w, ny.w, fy.w, nz.w, fz.w, oi, inv, tmin, best, t3);
        r0 = __float_as_int(rf.x); r1 = __float_as_int(rf.y); r2 = __float_as_int(rf.z); r3 = __float_as_int(rf.w);
    }
    // pushes and the pop below touch entries <= sp + 3: plain LDS accesses when no lane of
    // the wave can reach a spill stack's global part (wave-uniform test; always for LdsStack)
    auto step = [&](auto st) {
        if (OCT && MODE != 2) {
            // closest-hit over an LDS octant copy, whose children are stored in the octant's
            // front-to-back order (trace_kernel's copy loop): continue with the first hit child and
            // push the other hit ones so that they pop in that order — no distance keys and no
            // sorting network (C2 4.50 -> 4.40 ms, C3 41.4 -> 40.4 ms; the closest (t, id) does not
            // depend on the visiting order).  Any-hit queries (MODE 2, below) continue with the
            // LAST hit child: back to front is 4.6 % faster at C2 than front to back for the
            // shadow rays (they end at the light, and an occluder near it ends the query)
            const bool p3 = h3 & (h0 | h1 | h2), p2 = h2 & (h0 | h1), p1 = h1 & h0;
            st.put(sp + S::kStep, r3); sp = stack_adv<S>(sp, p3);
            st.put(sp + S::kStep, r2); sp = stack_adv<S>(sp, p2);
            st.put(sp + S::kStep, r1); sp = stack_adv<S>(sp, p1);
            const int tp = st.get(sp);
            const bool any_hit = h0 | h1 | h2 | h3;
            cur = h0 ? r0 : (h1 ? r1 : (h2 ? r2 : (h3 ? r3 : tp)));
            sp -= any_hit ? 0 : S::kStep;
        } else if (MODE == 2) {
            st.put(sp + S::kStep, r0); sp = stack_adv<S>(sp, h0);
            st.put(sp + S::kStep, r1); sp = stack_adv<S>(sp, h1);
            st.put(sp + S::kStep, r2); sp = stack_adv<S>(sp, h2);
            int top = st.get(sp);
            cur = h3 ? r3 : top;
            sp -= h3 ? 0 : S::kStep;
        } else {
            // nearest hit child first by a 3-comparator tournament on the entry distances
            // (misses count as +inf, a hit's distance is finite); the three others are pushed
            // when hit, i.e. when their key is finite: the loser of each pair, then the loser
            // of the final.  Keys and masks stay floats / lane masks (no 0/1 integers).
            // any-hit lanes of a mixed wave (MODE 0, global scenes): farthest hit child first —
            // keys negated (entry distances are >= tmin > 0; misses stay +inf).  A shadow ray ends
            // at the light, and an occluder near that end ends the query: C4 18.85 -> 18.67 ms
            // (the LDS scenes' shadow iterations go back to front for the same reason, MODE 2)
            if (MODE == 0 && any_lane) { t0 = -t0; t1 = -t1; t2 = -t2; t3 = -t3; }
            const float k0 = h0 ? t0 : INFINITY, k1 = h1 ? t1 : INFINITY;
            const float k2 = h2 ? t2 : INFINITY, k3 = h3 ? t3 : INFINITY;
            const bool m01 = k1 < k0, m23 = k3 < k2;
            const float a = m01 ? k1 : k0, xb = m01 ? k0 : k1;
            const float c = m23 ? k3 : k2, xd = m23 ? k2 : k3;
            const int ra = m01 ? r1 : r0, rb = m01 ? r0 : r1;
            const int rc = m23 ? r3 : r2, rd = m23 ? r2 : r3;
            const bool m = c < a;
            const int rn = m ? rc : ra, rl = m ? ra : rc;
            const float xn = m ? c : a, xl = m ? a : c;
            st.put(sp + S::kStep, rb); sp += xb < INFINITY ? S::kStep : 0;
            st.put(sp + S::kStep, rd); sp += xd < INFINITY ? S::kStep : 0;
            st.put(sp + S::kStep, rl); sp += xl < INFINITY ? S::kStep : 0;
            const int tp = st.get(sp);
            const bool any_hit = xn < INFINITY;
            cur = any_hit ? rn : tp;
            sp -= any_hit ? 0 : S::kStep;
        }
    };
    if (stk.lds_only(sp + 3 * S::kStep)) step(stk.lds());
    else step(stk);
}

// One inner-node visit of the eight-wide tree of an LDS-resident scene (prt_internal.h Bvh8Host; OCT
// only, MODE 1 or 2).  `nodes` is the block's octant copy (copy_octant_nodes8): copy k of a node is 14
// float4 — nx, fx, ny, fy, nz, fz of children 0-3, the same six of children 4-7, two ref quads — with the
// eight children in k's front-to-back order; node stride 112 float4, `sx` = the query's copy offset 14 k.
// The visit tests one group of four at a time: the first group's planes are dead before the second's are
// needed, so only the eight refs and the eight hit masks (lane masks) span it.
// Closest-hit (MODE 1): continues with the first hit child in stored order and pushes the other hit ones
// r7 .. r1, so that they pop front to back; any-hit (MODE 2): pushes r0 .. r6 by their hit flags and
// continues with r7 if hit, else pops (back to front), both as visit_node4 does over its octant copies.
// Pushes are unconditional writes above the top (<= 7 above the entry top, Bvh8Host::stack_need).
template <bool STATS, int MODE, class S>
__device__ __forceinline__ void visit_node8(const float4* __restrict__ nodes, int& cur, int& sp, S stk, V3 inv, V3 oi,
                                            int sx, float tmin, float best, Counters& cn) {
    static_assert(MODE == 1 || MODE == 2, "the eight-wide visit has no mixed-kind form");
    const LdsF4* nl = as_lds(nodes) + (int)(__umul24((uint32_t)cur, 112u) + (uint32_t)sx);
    if (STATS) { cn.nodes++; cn.it_inner++; }
    bool h[8];
    float tn;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const float4 nx = lds4(nl, 6 * g), fx = lds4(nl, 6 * g + 1), ny = lds4(nl, 6 * g + 2);
        const float4 fy = lds4(nl, 6 * g + 3), nz = lds4(nl, 6 * g + 4), fz = lds4(nl, 6 * g + 5);
        h[4 * g] = slab_nf(nx.x, fx.x, ny.x, fy.x, nz.x, fz.x, oi, inv, tmin, best, tn);
        h[4 * g + 1] = slab_nf(nx.y, fx.y, ny.y, fy.y, nz.y, fz.y, oi, inv, tmin, best, tn);
        h[4 * g + 2] = slab_nf(nx.z, fx.z, ny.z, fy.z, nz.z, fz.z, oi, inv, tmin, best, tn);
        h[4 * g + 3] = slab_nf(nx.w, fx.w, ny.w, fy.w, nz.w, fz.w, oi, inv, tmin, best, tn);
    }
    const float4 ra = lds4(nl, 12), rb = lds4(nl, 13);
    const int r[8] = {__float_as_int(ra.x), __float_as_int(ra.y), __float_as_int(ra.z), __float_as_int(ra.w),
                      __float_as_int(rb.x), __float_as_int(rb.y), __float_as_int(rb.z), __float_as_int(rb.w)};
    if (MODE == 2) {
#pragma unroll
        for (int k = 0; k < 7; ++k) { stk.put(sp + S::kStep, r[k]); sp = stack_adv<S>(sp, h[k]); }
        const int top = stk.get(sp);
        cur = h[7] ? r[7] : top;
        sp -= h[7] ? 0 : S::kStep;
    } else {
        // e[k]: some child before k is hit, i.e. k is not the one the visit continues with
        bool e[8];
        e[0] = false;
#pragma unroll
        for (int k = 1; k < 8; ++k) e[k] = e[k - 1] | h[k - 1];
#pragma unroll
        for (int k = 7; k >= 1; --k) { stk.put(sp + S::kStep, r[k]); sp = stack_adv<S>(sp, h[k] & e[k]); }
        int nxt = stk.get(sp);
#pragma unroll
        for (int k = 7; k >= 0; --k) nxt = h[k] ? r[k] : nxt;
        cur = nxt;
        sp -= (e[7] | h[7]) ? 0 : S::kStep;
    }
}

// MODE 0: per-lane query kind (`any` may differ between lanes); 1: every lane
// closest-hit; 2: every lane any-hit (phase-aligned shadow iterations).  Any-hit
// queries need no visiting order, so mode 2 skips the sorting network (visit_node4).
// W: children per node of the tree at `nodes`: 4 (the BVH4 in every form), or 8 (OCT only: the block's
// octant copy of an LDS-resident scene's BVH8, visit_node8).  Leaves, the suspended state and the
// watchdog are the same for both.
template <bool STATS, int MODE, class S, bool QN = false, bool RES = false, bool OCT = false, int W = 4>
__device__ __forceinline__ bool traverse_ww4(const float4* __restrict__ nodes, const float4* __restrict__ tris, V3 o,
                                             V3 d, float tmin, float tmax, bool any_lane, S stk, int& hit_id,
                                             float& hit_t, Counters& cn, TState* tsp = nullptr, int min_lanes = 0,
                                             int* fault = nullptr, int leaf_break = 0, int leaf_exit = 0,
                                             uint32_t guard_lim = kGuardTrips) {
    const bool any = MODE == 0 ? any_lane : MODE == 2;
    const V3 inv = ray_inv(d);
    V3 oi = o * inv;
    // near plane index per axis (0 = lo, 1 = hi) from the sign of 1/d
    int sx = __float_as_int(inv.x) < 0 ? 1 : 0, sy = __float_as_int(inv.y) < 0 ? 1 : 0,
        sz = __float_as_int(inv.z) < 0 ? 1 : 0;
    static_assert(W == 4 || (W == 8 && OCT && !QN), "the eight-wide tree exists as LDS octant copies only");
    if (OCT) sx = (W == 8 ? 14 : 7) * (sx | (sy << 1) | (sz << 2));   // octant copy offset (visit_node4 / 8)
    TState ts;
    if (RES) ts = *tsp;
    else tstate_init(ts, stk, tmax);
    float best = ts.best;
    int best_id = ts.best_id;
    uint32_t guard = 0;
    int sp = ts.sp;
    int cur = ts.cur;
    int leaf = ts.leaf;
    do {
        while (cur >= 0 && cur != S::kSent) {
            if constexpr (W == 8) visit_node8<STATS, MODE, S>(nodes, cur, sp, stk, inv, oi, sx, tmin, best, cn);
            else visit_node4<STATS, MODE, S, QN, OCT>(nodes, cur, sp, stk, inv, oi, sx, sy, sz, tmin, best, cn, any);
            if (STATS) wave_tick(cn.wi, cn.li);
            if (STATS) cn.max_sp = max(cn.max_sp, (uint32_t)(stk.depth(sp) + 1));
            if (cur < 0 && leaf >= 0) {   // postpone the leaf, keep descending
                leaf = cur;
                cur = stk.get(sp);
                sp -= S::kStep;
            }
            // leave for the leaf phase once at most `leaf_break` of the lanes still
            // descending have no postponed leaf (0: all of them hold one)
            if (__popcll(__ballot(leaf >= 0)) <= (uint32_t)leaf_break) break;
        }
        while (leaf < 0) {
            int v = -leaf - 1;
            int first = v >> 3, cnt = (v & 7) + 1;
            if (STATS) {
                cn.it_leaf++;
                // wave-level triangle-loop trips of this leaf trip (max leaf size over the lanes)
                int mc = 8;
                while (mc > 1 && !__ballot(cnt >= mc)) --mc;
                if (__builtin_amdgcn_readfirstlane(__lane_id()) == __lane_id()) cn.w_tri += mc;
            }
            for (int k = 0; k < cnt; ++k) {
                float4 q0, q1, q2;
                if constexpr (OCT) {
                    const LdsF4* tp = as_lds(tris) + (int)__umul24((uint32_t)(first + k), 3u);
                    q0 = lds4(tp, 0); q1 = lds4(tp, 1); q2 = lds4(tp, 2);
                } else {
                    const float4* tp = tris + (size_t)(first + k) * 3;
                    q0 = tp[0]; q1 = tp[1]; q2 = tp[2];
                }
                int id = __float_as_int(q0.w);
                float t;
                if (STATS) { cn.tris++; wave_tick(cn.wl, cn.ll); }
                if (mt_u(xyz(q0), xyz(q1), xyz(q2), o, d, tmin, best, id, best_id, any, t)) {
                    best = t;
                    best_id = id;
                    if (any) { cur = S::kSent; break; }
                }
            }
            if (any && best_id >= 0) { leaf = 0; break; }
            leaf = cur;
            if (cur < 0) {
                cur = stk.get(sp);
                sp -= S::kStep;
            }
            // back to the inner phase once at most `leaf_exit` lanes still hold a leaf
            // (they keep it postponed); 0: drain every lane's chain of leaves first
            if (__popcll(__ballot(leaf < 0)) <= (uint32_t)leaf_exit) break;
        }
        if (RES && (cur != S::kSent || leaf < 0) && __popcll(__ballot(true)) < min_lanes) break;
        // watchdog: a traversal revisiting nodes forever (corrupt tree) ends the query and
        // raises the fault flag that the host turns into an error, instead of hanging the GPU
        if (++guard > guard_lim) {
            if (fault) atomicOr(fault, 1);
            cur = S::kSent;
            leaf = 0;
        }
    } while (cur != S::kSent || leaf < 0);
    hit_id = best_id;
    hit_t = best;
    if (RES) {
        tsp->cur = cur; tsp->leaf = leaf; tsp->sp = sp; tsp->best_id = best_id; tsp->best = best;
        return !(cur != S::kSent || leaf < 0);
    }
    return best_id >= 0;
}

}  // namespace
}  // namespace prt

// prt_lbvh.hip — a resident scene's trees built from scratch on the device (prt_scene_rebuild, prt_scene.cpp;
// DESIGN.md §14): Morton codes of the triangles' centroids, a stable radix sort, the binary radix tree of
// Karras 2012 over the sorted keys (one thread per inner node, nobody waits for anybody), and the wide tree
// emitted top-down, one launch group per level, for four and eight children per node.  The boxes come afterwards
// from prt_refit.hip's launches.  No kernel of this file reads what another workgroup of the same launch wrote:
// a kernel boundary orders every stage after the one before it (the XCDs' L2s are not coherent within a
// launch).  The sort, the centroid reduction and the per-level scan are rocPRIM's.  The codes are restated in
// NumPy bit for bit (tests/lbvh_ref.py), so the unit is built with the library's -ffp-contract=off and every f32
// step below stands in a fixed order.
#include "prt_lbvh.h"

#include <cstring>   // before rocPRIM: its texture iterator calls memset unqualified

#include <rocprim/rocprim.hpp>

#include "prt_bvh_util.h"
#include "prt_internal.h"

namespace prt {
namespace {

constexpr int kLbvhBlock = 256;

inline unsigned lbvh_grid(int64_t n) { return (unsigned)((n + kLbvhBlock - 1) / kLbvhBlock); }

// ---------------------------------------------------------------- stage 1: codes
struct CenBox { float lo[3], hi[3]; };

struct CenLoad {
    const float* cen;
    __host__ __device__ CenBox operator()(size_t t) const {
        CenBox b;
        for (int k = 0; k < 3; ++k) b.lo[k] = b.hi[k] = cen[3 * t + k];
        return b;
    }
};
struct CenUnion {
    __host__ __device__ CenBox operator()(const CenBox& x, const CenBox& y) const {
        CenBox b;
        for (int k = 0; k < 3; ++k) {
            b.lo[k] = y.lo[k] < x.lo[k] ? y.lo[k] : x.lo[k];
            b.hi[k] = x.hi[k] < y.hi[k] ? y.hi[k] : x.hi[k];
        }
        return b;
    }
};
using CenIter = rocprim::transform_iterator<rocprim::counting_iterator<size_t>, CenLoad, CenBox>;

__global__ void __launch_bounds__(kLbvhBlock)
lbvh_centroid_kernel(const float* __restrict__ tri_v, int64_t n, float* __restrict__ cen) {
    const int64_t t = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (t >= n) return;
    const float* p = tri_v + 9 * t;
    for (int k = 0; k < 3; ++k) {
        // the slot bounds as refit_tris_kernel takes them, then their midpoint
        const float lo01 = p[3 + k] < p[k] ? p[3 + k] : p[k], hi01 = p[k] < p[3 + k] ? p[3 + k] : p[k];
        const float lo = p[6 + k] < lo01 ? p[6 + k] : lo01, hi = hi01 < p[6 + k] ? p[6 + k] : hi01;
        cen[3 * t + k] = (lo + hi) * 0.5f;
    }
}

// bits 0..9 of v to bits 0, 3, 6, ..., 27
__device__ inline uint32_t spread3(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__global__ void __launch_bounds__(kLbvhBlock)
lbvh_morton_kernel(const float* __restrict__ cen, const float* __restrict__ cbox, int64_t n,
                   uint32_t* __restrict__ codes, uint32_t* __restrict__ ids) {
    const int64_t t = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (t >= n) return;
    uint32_t q[3];
    for (int k = 0; k < 3; ++k) {
        const float ext = cbox[3 + k] - cbox[k];
        q[k] = 0;
        if (ext > 0.0f) {
            const float u = (cen[3 * t + k] - cbox[k]) / ext;   // in [0, 1]
            const int g = (int)(u * 1024.0f);
            q[k] = (uint32_t)(g > 1023 ? 1023 : g);
        }
    }
    codes[t] = (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
    ids[t] = (uint32_t)t;
}

// ---------------------------------------------------------------- stage 2: keys
__global__ void __launch_bounds__(kLbvhBlock)
lbvh_keys_kernel(const uint32_t* __restrict__ codes_sorted, int64_t n, uint64_t* __restrict__ keys) {
    const int64_t s = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (s >= n) return;
    keys[s] = ((uint64_t)codes_sorted[s] << 32) | (uint64_t)s;
}

// ---------------------------------------------------------------- stage 3: the binary radix tree
// length of the common prefix of keys i and j, -1 for a j outside the array (Karras 2012, δ); the keys differ
__device__ inline int lbvh_delta(const uint64_t* keys, int64_t n, int64_t i, int64_t j) {
    if (j < 0 || j >= n) return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));
}

__global__ void __launch_bounds__(kLbvhBlock)
lbvh_topology_kernel(const uint64_t* __restrict__ keys, int64_t n, int32_t* __restrict__ split) {
    const int64_t i = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (i >= n - 1) return;
    const int64_t d = lbvh_delta(keys, n, i, i + 1) > lbvh_delta(keys, n, i, i - 1) ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    split[i] = (int32_t)(i + s * d + (d < 0 ? -1 : 0));
}

// ---------------------------------------------------------------- stage 4: the wide tree, level by level
// The children of the wide node over [a, b] (inner node idx of the binary tree): log2(kWidth) rounds, each
// splitting every range of more than max_leaf slots in two.  Returns their number; ca / cb / ci as LbvhItem's.
// The split is held inside [a, b - 1], so both halves are ranges of [a, b] whatever split[] holds.
template <int kWidth>
__device__ inline int wide_children(int32_t a, int32_t b, int32_t idx, const int32_t* __restrict__ split, int max_leaf,
                                    int32_t* ca, int32_t* cb, int32_t* ci) {
    if (b < a) return 0;
    int n = 1;
    ca[0] = a; cb[0] = b; ci[0] = idx;
    for (int round = 1; round < kWidth; round *= 2) {
        int32_t ta[kWidth], tb[kWidth], ti[kWidth];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            if (cb[k] - ca[k] + 1 <= max_leaf) {
                ta[m] = ca[k]; tb[m] = cb[k]; ti[m] = ci[k]; ++m;
            } else {
                int32_t s = split[ci[k]];
                s = s < ca[k] ? ca[k] : s > cb[k] - 1 ? cb[k] - 1 : s;
                ta[m] = ca[k]; tb[m] = s; ti[m] = s; ++m;
                ta[m] = s + 1; tb[m] = cb[k]; ti[m] = s + 1; ++m;
            }
        }
        for (int k = 0; k < m; ++k) { ca[k] = ta[k]; cb[k] = tb[k]; ci[k] = ti[k]; }
        n = m;
    }
    return n;
}

__global__ void lbvh_root_kernel(LbvhItem* __restrict__ items, int64_t n, int32_t* __restrict__ max_anc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        items[0] = LbvhItem{0, (int32_t)(n - 1), 0, 0};
        *max_anc = 0;
    }
}

template <int kWidth>
__global__ void __launch_bounds__(kLbvhBlock)
lbvh_count_kernel(const LbvhItem* __restrict__ level, int64_t n_items, const int32_t* __restrict__ split, int max_leaf,
                  int32_t* __restrict__ cnt) {
    const int64_t j = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (j == n_items) cnt[j] = 0;   // the scan's last output is then the level's total
    if (j >= n_items) return;
    const LbvhItem it = level[j];
    int32_t ca[kWidth], cb[kWidth], ci[kWidth];
    const int n = wide_children<kWidth>(it.a, it.b, it.idx, split, max_leaf, ca, cb, ci);
    int inner = 0;
    for (int k = 0; k < n; ++k) inner += cb[k] - ca[k] + 1 > max_leaf ? 1 : 0;
    cnt[j] = inner;
}

template <int kWidth>
__global__ void __launch_bounds__(kLbvhBlock)
lbvh_scatter_kernel(LbvhItem* __restrict__ items, int64_t base, int64_t n_items, int64_t next_base,
                    const int32_t* __restrict__ split, int max_leaf, const int32_t* __restrict__ off,
                    int32_t* __restrict__ child0, int32_t* __restrict__ max_anc) {
    const int64_t j = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    int32_t anc = 0;
    if (j < n_items) {
        const LbvhItem it = items[base + j];
        int32_t ca[kWidth], cb[kWidth], ci[kWidth];
        const int n = wide_children<kWidth>(it.a, it.b, it.idx, split, max_leaf, ca, cb, ci);
        int64_t at = next_base + off[j];
        child0[base + j] = (int32_t)at;
        for (int k = 0; k < n; ++k)
            if (cb[k] - ca[k] + 1 > max_leaf) items[at++] = LbvhItem{ca[k], cb[k], ci[k], it.anc + n - 1};
        anc = it.anc;
    }
    // one atomic per wave, every lane of it here: the largest anc of the wave's 64 items
    for (int step = 32; step >= 1; step /= 2) {
        const int32_t other = __shfl_xor(anc, step);
        anc = other > anc ? other : anc;
    }
    if ((threadIdx.x & 63) == 0 && anc > 0) atomicMax(max_anc, anc);
}

template <int kWidth>
__global__ void __launch_bounds__(kLbvhBlock)
lbvh_emit_kernel(const LbvhItem* __restrict__ items, const int32_t* __restrict__ child0, int64_t n_nodes,
                 const int32_t* __restrict__ split, int max_leaf, float* __restrict__ nodes) {
    constexpr int kNode = kWidth == 4 ? kNode4F4 * 4 : kNode8F4 * 4;
    const int64_t i = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (i >= n_nodes) return;
    const LbvhItem it = items[i];
    int32_t ca[kWidth], cb[kWidth], ci[kWidth];
    const int n = wide_children<kWidth>(it.a, it.b, it.idx, split, max_leaf, ca, cb, ci);
    float* f = nodes + (size_t)i * kNode;
    for (int k = 0; k < kNode; ++k) f[k] = 0.0f;
    int32_t next = child0[i];
    for (int k = 0; k < kWidth; ++k) {
        const int at = (k / 4) * 24 + k % 4;
        for (int a = 0; a < 3; ++a) {
            f[at + (2 * a) * 4] = INFINITY;
            f[at + (2 * a + 1) * 4] = -INFINITY;
        }
        int32_t ref = kEmptyRef;
        if (k < n) ref = cb[k] - ca[k] + 1 > max_leaf ? next++ : leaf_ref(ca[k], cb[k] - ca[k] + 1);
        f[6 * kWidth + k] = bits<float>(ref);
    }
}

__global__ void __launch_bounds__(kLbvhBlock) lbvh_iota_kernel(int32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kLbvhBlock + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

inline CenIter cen_iter(const float* cen) {
    return CenIter(rocprim::counting_iterator<size_t>(0), CenLoad{cen});
}
inline CenBox cen_none() { return CenBox{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }

}  // namespace

hipError_t lbvh_temp_bytes(int64_t n, size_t* bytes) {
    const size_t m = (size_t)(n > 0 ? n : 1);
    size_t need = 0, most = 0;
    hipError_t e = rocprim::reduce(nullptr, need, cen_iter(nullptr), (CenBox*)nullptr, cen_none(), m, CenUnion());
    if (e != hipSuccess) return e;
    most = need;
    e = rocprim::radix_sort_pairs(nullptr, need, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, m, 0u, 30u);
    if (e != hipSuccess) return e;
    most = need > most ? need : most;
    // a level holds at most n / 2 nodes (each covers two slots or more), and the root's level one
    e = rocprim::exclusive_scan(nullptr, need, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, m / 2 + 2,
                                rocprim::plus<int32_t>());
    if (e != hipSuccess) return e;
    *bytes = (need > most ? need : most) + 256;
    return hipSuccess;
}

hipError_t launch_lbvh_codes(const float* tri_v, int64_t n, float* cen, float* cbox, uint32_t* codes, uint32_t* ids,
                             void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lbvh_centroid_kernel, dim3(lbvh_grid(n)), dim3(kLbvhBlock), 0, stream, tri_v, n, cen);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::reduce(temp, temp_bytes, cen_iter(cen), (CenBox*)cbox, cen_none(), (size_t)n, CenUnion(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_morton_kernel, dim3(lbvh_grid(n)), dim3(kLbvhBlock), 0, stream, cen, cbox, n, codes, ids);
    return hipGetLastError();
}

hipError_t launch_lbvh_sort(const uint32_t* codes, const uint32_t* ids, int64_t n, uint32_t* codes_sorted,
                            int32_t* order, uint64_t* keys, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, codes, codes_sorted, ids, (uint32_t*)order, (size_t)n, 0u,
                                             30u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lbvh_keys_kernel, dim3(lbvh_grid(n)), dim3(kLbvhBlock), 0, stream, codes_sorted, n, keys);
    return hipGetLastError();
}

hipError_t launch_lbvh_topology(const uint64_t* keys, int64_t n, int32_t* split, hipStream_t stream) {
    if (n < 2) return hipSuccess;
    hipLaunchKernelGGL(lbvh_topology_kernel, dim3(lbvh_grid(n - 1)), dim3(kLbvhBlock), 0, stream, keys, n, split);
    return hipGetLastError();
}

hipError_t launch_lbvh_root(LbvhItem* items, int64_t n, int32_t* max_anc, hipStream_t stream) {
    hipLaunchKernelGGL(lbvh_root_kernel, dim3(1), dim3(64), 0, stream, items, n, max_anc);
    return hipGetLastError();
}

hipError_t launch_lbvh_level(int width, LbvhItem* items, int64_t base, int64_t n_items, int64_t next_base,
                             const int32_t* split, int max_leaf, int32_t* cnt, int32_t* off, int32_t* child0,
                             int32_t* max_anc, void* temp, size_t temp_bytes, hipStream_t stream) {
    if (n_items <= 0) return hipSuccess;
    const dim3 grid(lbvh_grid(n_items + 1)), block(kLbvhBlock);
    if (width == 8)
        hipLaunchKernelGGL(lbvh_count_kernel<8>, grid, block, 0, stream, items + base, n_items, split, max_leaf, cnt);
    else
        hipLaunchKernelGGL(lbvh_count_kernel<4>, grid, block, 0, stream, items + base, n_items, split, max_leaf, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp, temp_bytes, (const int32_t*)cnt, off, (int32_t)0, (size_t)n_items + 1,
                                rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return e;
    if (width == 8)
        hipLaunchKernelGGL(lbvh_scatter_kernel<8>, grid, block, 0, stream, items, base, n_items, next_base, split,
                           max_leaf, off, child0, max_anc);
    else
        hipLaunchKernelGGL(lbvh_scatter_kernel<4>, grid, block, 0, stream, items, base, n_items, next_base, split,
                           max_leaf, off, child0, max_anc);
    return hipGetLastError();
}

hipError_t launch_lbvh_emit(int width, const LbvhItem* items, const int32_t* child0, int64_t n_nodes,
                            const int32_t* split, int max_leaf, float* nodes, hipStream_t stream) {
    if (n_nodes <= 0) return hipSuccess;
    const dim3 grid(lbvh_grid(n_nodes)), block(kLbvhBlock);
    if (width == 8)
        hipLaunchKernelGGL(lbvh_emit_kernel<8>, grid, block, 0, stream, items, child0, n_nodes, split, max_leaf, nodes);
    else
        hipLaunchKernelGGL(lbvh_emit_kernel<4>, grid, block, 0, stream, items, child0, n_nodes, split, max_leaf, nodes);
    return hipGetLastError();
}

hipError_t launch_lbvh_iota(int32_t* out, int64_t n, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lbvh_iota_kernel, dim3(lbvh_grid(n)), dim3(kLbvhBlock), 0, stream, out, n);
    return hipGetLastError();
}

}  // namespace prt

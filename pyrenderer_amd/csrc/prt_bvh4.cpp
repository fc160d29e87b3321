// prt_bvh4.cpp — what consumes the flat BVH2 (BvhHost, prt_bvh.cpp): its collapse into four-wide
// nodes (and eight-wide ones for LDS-resident scenes), SAH-optimal (DpCollapse) or greedy, and the 8-bit
// quantisation of the four-wide nodes.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prt_bvh_util.h"
#include "prt_internal.h"

namespace prt {
namespace {

constexpr int kNode4 = kNode4F4 * 4;  // floats of one four-wide node
// Cost of one visit of a `width`-wide node in the DP, in four-wide visits (ct is relative to those): the
// eight-wide visit tests two groups of four boxes and pushes up to seven children, 159 (closest-hit) and
// 129 (any-hit) VALU instructions against 77 and 69 in the pooled kernel's listing
constexpr double visit_cost(int width) { return width == 4 ? 1.0 : 2.0; }

// The collapse's knobs, read once per collapse: the env variable through atoi / atof, then the clamp.
struct CollapseKnobs {
    bool dp = true;     // PRT_BVH4_DP  0 = greedy open-the-largest instead of the SAH-optimal cut (config 2:
                        //              24.8 node visits per sample against 22.7)
    double ct = 0.5;    // PRT_DP_CT    >= 0: cost of one triangle test relative to one node visit
    int leaf_cap = 0;   // PRT_DP_LEAF  0..8: subtrees of <= this many triangles may merge into one leaf
    CollapseKnobs() {
        if (const char* e = std::getenv("PRT_BVH4_DP")) dp = std::atoi(e) != 0;
        if (const char* e = std::getenv("PRT_DP_CT")) ct = std::max(0.0, std::atof(e));
        if (const char* e = std::getenv("PRT_DP_LEAF")) leaf_cap = std::max(0, std::min(kMaxLeaf, std::atoi(e)));
    }
};

struct Child {
    float lo[3], hi[3];
    int32_t ref;
    bool empty;
    double area() const { return box_area(lo, hi); }
};

inline Child child_of(const float* n2, int side) {
    Child c;
    const float* b = n2 + 6 * side;
    c.lo[0] = b[0]; c.hi[0] = b[1]; c.lo[1] = b[2]; c.hi[1] = b[3]; c.lo[2] = b[4]; c.hi[2] = b[5];
    c.ref = bits<int32_t>(n2[12 + side]);
    c.empty = !(c.lo[0] <= c.hi[0]);
    return c;
}

// SAH-optimal collapse of the BVH2 into `width`-wide nodes (Ylitie et al. 2017's dynamic program).
// Expected cost of a tree = sum over wide nodes of area x visit_cost(width) (one visit) + sum
// over leaf entries of area x ct x triangles.  cost[i][k] (k = 2..width) = least cost of representing
// inner BVH2 node i's subtree by exactly k entries of one wide node, the subtrees below those
// entries included; cost[i][1] = least cost of i as one entry: its own wide node, or (subtrees of
// <= leaf_cap triangles) one leaf of its whole triangle range.  split[i][k] = entries taken from
// the left child.
struct DpCollapse {
    const int kWidth;             // children of one collapsed node
    const int kStride;            // table row of one node: k = 0..kWidth
    std::vector<double> cost;     // n2 * kStride
    std::vector<int8_t> split;    // n2 * kStride
    std::vector<double> area;     // n2: surface area of inner node i
    std::vector<int64_t> first;   // n2: triangle range of i's subtree (BVH order)
    std::vector<int32_t> count;   //     (-1: not one contiguous range)
    std::vector<uint8_t> as_leaf; // n2: cost[i][1] is the merged leaf
    const BvhHost& b2;
    double ct;
    int leaf_cap;
    DpCollapse(const BvhHost& b, double ct_, int leaf_cap_, int width)
        : kWidth(width), kStride(width + 1), b2(b), ct(ct_), leaf_cap(leaf_cap_) {
        const int64_t n2 = b2.n_nodes;
        cost.assign((size_t)n2 * kStride, INFINITY);
        split.assign((size_t)n2 * kStride, 0);
        area.assign((size_t)n2, 0.0);
        first.assign((size_t)n2, 0);
        count.assign((size_t)n2, -1);
        as_leaf.assign((size_t)n2, 0);
        for (int64_t i = 0; i < n2; ++i)
            for (int s = 0; s < 2; ++s) {
                Child c = child_of(node(i), s);
                if (c.ref >= 0 && !c.empty) area[(size_t)c.ref] = c.area();
            }
        if (n2 > 0) {   // the root's box is the union of its children's
            Child a = child_of(node(0), 0), b = child_of(node(0), 1);
            Child u = a;
            for (int k = 0; k < 3; ++k) {
                if (!b.empty) { u.lo[k] = std::min(u.lo[k], b.lo[k]); u.hi[k] = std::max(u.hi[k], b.hi[k]); }
            }
            area[0] = a.empty ? 0.0 : u.area();
        }
        solve();
    }
    const float* node(int64_t i) const { return b2.nodes.data() + (size_t)i * 16; }
    // fills the tables bottom-up: preorder ids, children follow their parent, so a reverse sweep
    void solve() {
        for (int64_t i = b2.n_nodes - 1; i >= 0; --i) {
            Child c[2] = {child_of(node(i), 0), child_of(node(i), 1)};
            double* ci = &cost[(size_t)i * kStride];
            for (int k = 2; k <= kWidth; ++k) {
                for (int a = c[0].empty ? 0 : 1; a <= k; ++a) {
                    int b = k - a;
                    if (c[1].empty ? b != 0 : b < 1) continue;
                    double v = side(c[0], a) + side(c[1], b);
                    if (v < ci[k]) { ci[k] = v; split[(size_t)i * kStride + k] = (int8_t)a; }
                }
            }
            // a single-leaf scene (one empty child) still gets a node of its one entry
            double best = c[1].empty ? side(c[0], 1) : INFINITY;
            for (int k = 2; k <= kWidth; ++k) best = std::min(best, ci[k]);
            ci[1] = area[(size_t)i] * visit_cost(kWidth) + best;
            int64_t f[2];
            int32_t m[2];
            for (int s = 0; s < 2; ++s) range(c[s], &f[s], &m[s]);
            if (m[0] >= 0 && m[1] >= 0 && f[0] + m[0] == f[1]) {
                first[(size_t)i] = f[0];
                count[(size_t)i] = m[0] + m[1];
                double leaf = area[(size_t)i] * ct * (double)(m[0] + m[1]);
                if (i > 0 && m[0] + m[1] <= leaf_cap && leaf < ci[1]) { ci[1] = leaf; as_leaf[(size_t)i] = 1; }
            }
        }
    }
    void range(const Child& c, int64_t* f, int32_t* m) const {
        if (c.empty) { *f = 0; *m = -1; return; }
        if (c.ref < 0) { *f = leaf_first(c.ref); *m = leaf_count(c.ref); return; }
        *f = first[(size_t)c.ref]; *m = count[(size_t)c.ref];
    }
    double side(const Child& c, int a) const {
        if (c.empty) return a == 0 ? 0.0 : INFINITY;
        if (a == 0) return INFINITY;
        if (c.ref < 0) return a == 1 ? c.area() * ct * (double)leaf_count(c.ref) : INFINITY;
        return cost[(size_t)c.ref * kStride + a];
    }
    // one entry: a BVH2 leaf, an inner node, or an inner node's subtree merged into one leaf
    Child entry(const Child& c) const {
        Child e = c;
        if (c.ref >= 0 && as_leaf[(size_t)c.ref]) e.ref = leaf_ref(first[(size_t)c.ref], count[(size_t)c.ref]);
        return e;
    }
    // entries of inner node i's k-entry cut (k >= 2)
    void expand(int32_t i, int k, std::vector<Child>* outc) const {
        Child c[2] = {child_of(node(i), 0), child_of(node(i), 1)};
        int a = split[(size_t)i * kStride + k];
        int parts[2] = {a, k - a};
        for (int s = 0; s < 2; ++s) {
            if (parts[s] == 0) continue;
            if (parts[s] == 1) outc->push_back(entry(c[s]));
            else expand(c[s].ref, parts[s], outc);
        }
    }
    // children of the wide node made from inner node i: its cheapest cut
    void children(int32_t i, std::vector<Child>* outc) const {
        const double* ci = &cost[(size_t)i * kStride];
        if (child_of(node(i), 1).empty) {
            Child c0 = child_of(node(i), 0);
            if (!c0.empty) outc->push_back(entry(c0));
            return;
        }
        int k = 2;
        for (int j = 3; j <= kWidth; ++j)
            if (ci[j] < ci[k]) k = j;
        expand(i, k, outc);
    }
};

// greedy children of the `width`-wide node made from inner node i: its two children, the inner one with
// the largest surface area opened again and again until the node is full
void greedy_children(const BvhHost& b2, int32_t i, int width, std::vector<Child>* ch) {
    for (int side = 0; side < 2; ++side) {
        Child c = child_of(b2.nodes.data() + (size_t)i * 16, side);
        if (!c.empty) ch->push_back(c);
    }
    while ((int)ch->size() < width) {
        int best = -1;
        double ba = -1.0;
        for (size_t k = 0; k < ch->size(); ++k)
            if ((*ch)[k].ref >= 0 && (*ch)[k].area() > ba) { ba = (*ch)[k].area(); best = (int)k; }
        if (best < 0) break;
        const float* m = b2.nodes.data() + (size_t)(*ch)[best].ref * 16;
        Child a = child_of(m, 0), b = child_of(m, 1);
        ch->erase(ch->begin() + best);
        if (!a.empty) ch->push_back(a);
        if (!b.empty) ch->push_back(b);
    }
}

// Writes the wide BVH (Bvh4Host: kWidth 4, Bvh8Host: kWidth 8) top-down from the root: `children(i, &ch)`
// names the entries of the node made from inner BVH2 node i, each inner entry gets the next node slot.
// Children go in groups of four: plane p (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z) of child k at float
// (k / 4) * 24 + 4 p + k % 4, the refs after the last group.
// anc = entries the traversal can hold for the node's strict ancestors: a visit continues
// with one hit child and pushes the others (<= children - 1), and LIFO order means the
// stack below a node holds only siblings of its ancestors (traverse_ww4)
template <int kWidth, class Host, class Chooser>
void emit_wide(const Chooser& children, Host* out) {
    constexpr int kNode = kWidth == 4 ? kNode4 : kNode8F4 * 4;   // floats of one node
    struct Item { int32_t b2node; int32_t slot; int32_t depth; int32_t anc; };
    std::vector<Item> work;
    out->nodes.clear();
    out->nodes.resize(kNode, 0.0f);
    out->n_nodes = 1;
    out->depth = 0;
    int32_t max_anc = 0;
    work.push_back({0, 0, 0, 0});
    std::vector<Child> ch;
    while (!work.empty()) {
        Item it = work.back();
        work.pop_back();
        ch.clear();
        children(it.b2node, &ch);
        float* f = out->nodes.data() + (size_t)it.slot * kNode;
        for (int k = 0; k < kWidth; ++k) {
            bool ok = k < (int)ch.size();
            const int at = (k / 4) * 24 + k % 4;
            for (int a = 0; a < 3; ++a) {
                // empty slot: inverted box (lo = +inf, hi = -inf) is missed by every ray
                // whose direction has one finite 1/d, whatever t_max (even NaN / inf)
                f[at + (2 * a) * 4] = ok ? ch[k].lo[a] : INFINITY;
                f[at + (2 * a + 1) * 4] = ok ? ch[k].hi[a] : -INFINITY;
            }
            // empty slot ref = the traversal sentinel: if a NaN ray ever "hits" it, the lane's
            // traversal ends instead of restarting at the root (a NaN ray hits nothing anyway)
            int32_t ref = kEmptyRef;
            if (ok) {
                if (ch[k].ref >= 0) {
                    ref = (int32_t)out->n_nodes++;
                    out->nodes.resize((size_t)out->n_nodes * kNode, 0.0f);
                    f = out->nodes.data() + (size_t)it.slot * kNode;   // storage may have moved
                    work.push_back({ch[k].ref, ref, it.depth + 1, it.anc + (int32_t)ch.size() - 1});
                } else {
                    ref = ch[k].ref;
                }
            }
            f[6 * kWidth + k] = bits<float>(ref);
        }
        out->depth = std::max(out->depth, it.depth);
        max_anc = std::max(max_anc, it.anc);
    }
    // the sentinel, the deepest node's ancestor entries, and the <= kWidth - 1 slots a visit writes
    // above the top unconditionally (visit_node4, visit_node8); <= (kWidth - 1) (depth + 1) + 1, the
    // per-level bound
    out->stack_need = 1 + max_anc + (kWidth - 1);
}

template <int kWidth, class Host>
void collapse_wide(const BvhHost& b2, Host* out) {
    const CollapseKnobs knobs;
    if (knobs.dp) {
        const DpCollapse dp(b2, knobs.ct, knobs.leaf_cap, kWidth);
        emit_wide<kWidth>([&](int32_t i, std::vector<Child>* ch) { dp.children(i, ch); }, out);
    } else {
        emit_wide<kWidth>([&](int32_t i, std::vector<Child>* ch) { greedy_children(b2, i, kWidth, ch); }, out);
    }
}

}  // namespace

void collapse_bvh4(const BvhHost& b2, Bvh4Host* out) { collapse_wide<4>(b2, out); }
void collapse_bvh8(const BvhHost& b2, Bvh8Host* out) { collapse_wide<8>(b2, out); }

void quantize_bvh4(const Bvh4Host& b4, float pad, std::vector<float>* out) {
    out->assign((size_t)b4.n_nodes * 16, 0.0f);
    for (int64_t n = 0; n < b4.n_nodes; ++n)
        quantize_node4(b4.nodes.data() + (size_t)n * kNode4, pad, out->data() + (size_t)n * 16);
}

}  // namespace prt

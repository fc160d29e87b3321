// prt_bvh.cpp — host-side binned-SAH BVH2 builder over triangles.
//
// The reference builds its BVH over *primitives* (median split in insertion
// order, accelerators/bvh_taichi.py:58-161) and brute-forces each primitive's
// triangles (mathematics/shapes.py:76-110).  That does not scale past a few
// primitives, so libprt builds a triangle-level SAH tree (the intent of the
// reference's unused CPU builder, accelerators/bvh.py:28-215, 12 buckets) and
// lays it out for the GPU: 64-B nodes with both child boxes, triangles as
// (v0, e1, e2) in leaf order.  Closest-hit results do not depend on the tree:
// ties resolve to the lowest original triangle index, which is also the
// reference's first-found order (leaves visited in insertion order).
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prt_bvh_util.h"
#include "prt_internal.h"

namespace prt {
namespace {

struct Box {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    float hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    void grow(const Box& b) {
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); }
    }
    void grow(const float* p) {
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); }
    }
    bool valid() const { return lo[0] <= hi[0]; }
    double area() const { return valid() ? box_area(lo, hi) : 0.0; }
};

struct TNode {
    Box box;
    int32_t left = -1, right = -1;   // temp node ids
    int64_t first = 0;
    int32_t count = 0;               // > 0 for leaves
};

constexpr int kMaxBins = 128;

// The builder's knobs: name, default, clamp and meaning of each in read_bvh_knobs, which reads them once
// per build.  knob(): the env variable through atoi / atof, then the clamp; the default when it is unset.
struct BvhKnobs { int bins, leaf_min, treelet; bool sbvh, verbose; double alpha, budget, ct, esc_beta; };

int knob(const char* name, int def, int lo, int hi) {
    const char* e = std::getenv(name);
    return e ? std::max(lo, std::min(hi, std::atoi(e))) : def;
}
double knob(const char* name, double def, double lo) {
    const char* e = std::getenv(name);
    return e ? std::max(lo, std::atof(e)) : def;
}

BvhKnobs read_bvh_knobs(int64_t n_tri, int max_leaf) {
    // scenes of >= 2^14 triangles (never LDS-resident) build finer: 64 SAH bins, early split clipping
    // above 128 x the mean box area, treelet restructuring (config 4: node visits 144.3 -> 138.1 per
    // sample against 32 bins / 64 x / no treelets, profiles/r05/treelet/; the treelets alone: BVH2 SAH
    // -3 %, node visits -2.1 %, 157.5 -> 154.6 ms per launch); the small LDS scenes keep the round-4
    // tree, whose BVH4 collapse visits fewer nodes there (Cornell: 22.7 vs 26.3 node visits per sample
    // with the restructured tree, profiles/r05/treelet/)
    const bool large = n_tri >= (1 << 14);
    BvhKnobs k;
    k.bins = knob("PRT_SAH_BINS", large ? 64 : 32, 2, kMaxBins);    // SAH bins per axis, object and spatial
    k.sbvh = knob("PRT_SBVH", 1, INT_MIN, INT_MAX) != 0;            // spatial splits (0 = off)
    k.alpha = knob("PRT_SBVH_ALPHA", 1e-5, 0.0);                    // ... tried above this overlap x the root's area
    k.budget = knob("PRT_SBVH_BUDGET", 1.3, 1.0);                   // ... until references = budget x the initial ones
    k.ct = knob("PRT_SAH_CT", 0.5, 0.0);                            // cost of a node step relative to a triangle test
    k.leaf_min = knob("PRT_LEAF_MIN", 2, 1, max_leaf);              // ranges this small always become leaves
    k.esc_beta = knob("PRT_ESC_BETA", large ? 128.0 : 64.0, 0.0);   // early split clipping above beta x mean area (0 = off)
    k.treelet = knob("PRT_TREELET", large ? 3 : 0, 0, 8);           // treelet restructuring passes (0 = off)
    k.verbose = std::getenv("PRT_BVH_VERBOSE") != nullptr;          // set: statistics on stderr
    return k;
}

// ---------------------------------------------------------- early split clipping
// A triangle far larger than the scene's typical one (the Cornell walls among config 4's
// million small cube faces) would otherwise sit deep in the tree and inflate the box of
// every ancestor to the wall's size, so every ray near the wall walks those subtrees
// (config 4: up to 2067 node visits in one query against 25 on average).  Such a
// triangle enters the build as several references, each the triangle clipped to one cell
// of a recursive midpoint split of its box (Ernst & Greiner 2007, "early split
// clipping").  The triangle record is the same for every reference, so traversal tests
// the same Moller-Trumbore on it, possibly more than once, and the closest (t, id) is
// unchanged; the reference boxes only have to cover the triangle, which they do: each
// is the bound of the triangle clipped to its cell (Sutherland-Hodgman in double),
// rounded outward to f32, and then padded like every other box.
struct RefBox { double lo[3], hi[3]; };

// bounds of triangle `t` (3 x xyz) clipped in double to box `c`; false when they do not meet
bool clip_bounds(const float* t, const RefBox& c, RefBox* out) {
    double poly[16][3], tmp[16][3];
    int n = 3;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) poly[i][k] = (double)t[3 * i + k];
    for (int ax = 0; ax < 3 && n > 0; ++ax)
        for (int side = 0; side < 2 && n > 0; ++side) {
            const double b = side == 0 ? c.lo[ax] : c.hi[ax];
            auto inside = [&](const double* p) { return side == 0 ? p[ax] >= b : p[ax] <= b; };
            int m = 0;
            for (int i = 0; i < n; ++i) {
                const double* a = poly[i];
                const double* q = poly[(i + 1) % n];
                const bool ia = inside(a), iq = inside(q);
                if (ia) { for (int k = 0; k < 3; ++k) tmp[m][k] = a[k]; ++m; }
                if (ia != iq && m < 15) {
                    const double u = (b - a[ax]) / (q[ax] - a[ax]);
                    for (int k = 0; k < 3; ++k) tmp[m][k] = a[k] + u * (q[k] - a[k]);
                    tmp[m][ax] = b;
                    ++m;
                }
            }
            n = m;
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k) poly[i][k] = tmp[i][k];
        }
    if (n == 0) return false;
    for (int k = 0; k < 3; ++k) { out->lo[k] = INFINITY; out->hi[k] = -INFINITY; }
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            out->lo[k] = std::min(out->lo[k], poly[i][k]);
            out->hi[k] = std::max(out->hi[k], poly[i][k]);
        }
    for (int k = 0; k < 3; ++k) {   // the polygon lies in the cell up to rounding
        out->lo[k] = std::max(out->lo[k], c.lo[k]);
        out->hi[k] = std::min(out->hi[k], c.hi[k]);
    }
    return true;
}

void split_refs(const float* t, const RefBox& cell, double thr, int depth, std::vector<RefBox>* out) {
    RefBox b;
    if (!clip_bounds(t, cell, &b)) return;
    if (box_area(b.lo, b.hi) <= thr || depth >= 12) {
        out->push_back(b);
        return;
    }
    int ax = 0;
    for (int k = 1; k < 3; ++k)
        if (b.hi[k] - b.lo[k] > b.hi[ax] - b.lo[ax]) ax = k;
    const double mid = 0.5 * (b.lo[ax] + b.hi[ax]);
    RefBox l = b, r = b;
    l.hi[ax] = mid;
    r.lo[ax] = mid;
    split_refs(t, l, thr, depth + 1, out);
    split_refs(t, r, thr, depth + 1, out);
}

inline Box outward_f32(const RefBox& r, const Box& tri_box) {
    Box b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = std::max(round_down_f32(r.lo[k]), tri_box.lo[k]);   // never beyond the triangle's own box
        b.hi[k] = std::min(round_up_f32(r.hi[k]), tri_box.hi[k]);
    }
    return b;
}

// Binned-SAH builder over references (a triangle, or an early-split-clipping piece of one), with
// spatial splits (Stich, Friedrich & Dietrich 2009, "Spatial Splits in Bounding Volume
// Hierarchies"; env PRT_SBVH=0 turns them off): where the best object split's two children overlap
// (their intersection's area > alpha x the root's), the node's box is also cut by `bins` planes per
// axis, every reference chopped into the bins it spans, and the cheaper of the two splits is taken.
// A reference straddling a spatial split plane goes to both sides as two references, each bounding
// the triangle's part on its side (its triangle clipped to the reference box and the side, bounds in
// double rounded outward to f32) — unless moving it whole to one side costs less (reference
// unsplitting).  Duplicates stop at a budget of references.  Every reference's record is its whole
// triangle, so a leaf tests the same Moller-Trumbore on it and the closest (t, id) is unchanged;
// the union of a triangle's reference boxes covers it.
// build() per node: bounds -> leaf test -> object_split -> spatial_split (where the children overlap)
// -> SAH leaf test -> partition_object / partition_spatial / median_halves -> recurse.
struct Builder {
    // the best plane of a search: references of bins <= split go left; boxes of the two sides
    struct Split { double cost = DBL_MAX; int axis = -1, split = -1; Box left, right; };
    using Refs = std::vector<int32_t>;
    const float* tv;           // triangle vertices (n_tri x 9)
    int max_leaf;
    BvhKnobs knobs;
    double min_overlap = 0.0;  // alpha x root area
    int64_t ref_budget = 0;    // spatial splits stop once the references reach this count
    std::vector<Box> tb;       // per reference: box
    std::vector<float> cen;    // per reference: box centre (3)
    Refs ref_tri;              // per reference: original triangle
    Refs order;                // leaf order of the references (output)
    std::vector<TNode> nodes;
    int32_t max_depth = 0;
    int64_t leaves = 0, spatial_splits = 0;

    void set_centre(int32_t r) {
        for (int a = 0; a < 3; ++a) cen[3 * (size_t)r + a] = 0.5f * (tb[(size_t)r].lo[a] + tb[(size_t)r].hi[a]);
    }
    // the part of reference r's triangle inside box `cell` (intersected with the reference's box),
    // rounded outward; false when empty
    bool clip_ref(int32_t r, double lo_ax, double hi_ax, int ax, Box* out) const {
        const float* t = tv + 9 * (size_t)ref_tri[(size_t)r];
        const Box& rb = tb[(size_t)r];
        RefBox cell;
        for (int a = 0; a < 3; ++a) { cell.lo[a] = rb.lo[a]; cell.hi[a] = rb.hi[a]; }
        cell.lo[ax] = std::max(cell.lo[ax], lo_ax);
        cell.hi[ax] = std::min(cell.hi[ax], hi_ax);
        if (!(cell.lo[ax] <= cell.hi[ax])) return false;
        RefBox cb;
        if (!clip_bounds(t, cell, &cb)) return false;
        Box tri_box;
        tri_box.grow(t); tri_box.grow(t + 3); tri_box.grow(t + 6);
        *out = outward_f32(cb, tri_box);
        // never beyond the reference's own box (the parent region)
        for (int a = 0; a < 3; ++a) {
            out->lo[a] = std::max(out->lo[a], rb.lo[a]);
            out->hi[a] = std::min(out->hi[a], rb.hi[a]);
        }
        return out->lo[0] <= out->hi[0] && out->lo[1] <= out->hi[1] && out->lo[2] <= out->hi[2];
    }
    static Box meet(const Box& a, const Box& b) {
        Box m;
        for (int k = 0; k < 3; ++k) { m.lo[k] = std::max(a.lo[k], b.lo[k]); m.hi[k] = std::min(a.hi[k], b.hi[k]); }
        for (int k = 0; k < 3; ++k)
            if (!(m.lo[k] <= m.hi[k])) return Box();
        return m;
    }
    // One axis of a binned SAH search: count_in[b] references start in bin b (left of every plane at or
    // after b), count_out[b] end there (right of every plane before b).  A plane replaces *best only
    // when strictly cheaper: ties go to the lowest axis, then the lowest plane.
    void sweep(int ax, const Box* bb, const int64_t* count_in, const int64_t* count_out, Split* best) const {
        Box rbx[kMaxBins];
        int64_t rc[kMaxBins];
        Box acc;
        int64_t c = 0;
        for (int b = knobs.bins - 1; b > 0; --b) {
            acc.grow(bb[b]); c += count_out[b];
            rbx[b] = acc; rc[b] = c;
        }
        Box lacc;
        int64_t lc = 0;
        for (int b = 0; b < knobs.bins - 1; ++b) {
            lacc.grow(bb[b]); lc += count_in[b];
            if (lc == 0 || rc[b + 1] == 0) continue;
            double cost = lacc.area() * (double)lc + rbx[b + 1].area() * (double)rc[b + 1];
            if (cost < best->cost) *best = Split{cost, ax, b, lacc, rbx[b + 1]};
        }
    }
    // object-split bin of reference r: its centre on the centroid box's axis, scale = bins / extent
    int centroid_bin(int32_t r, int ax, const Box& cb, double scale) const {
        int b = (int)(((double)cen[3 * (size_t)r + ax] - cb.lo[ax]) * scale);
        return std::min(std::max(b, 0), knobs.bins - 1);
    }
    double centroid_scale(const Box& cb, int ax) const { return knobs.bins / (double)(cb.hi[ax] - cb.lo[ax]); }
    // binned SAH object split over the three axes (cb: the centroids' box)
    Split object_split(const Refs& refs, const Box& cb) const {
        Split best;
        for (int ax = 0; ax < 3; ++ax) {
            if (!(cb.hi[ax] - cb.lo[ax] > 0.0f)) continue;
            Box bb[kMaxBins];
            int64_t cnt[kMaxBins] = {0};
            const double scale = centroid_scale(cb, ax);
            for (int32_t r : refs) {
                const int b = centroid_bin(r, ax, cb, scale);
                cnt[b]++;
                bb[b].grow(tb[(size_t)r]);
            }
            sweep(ax, bb, cnt, cnt, &best);
        }
        return best;
    }
    void partition_object(Refs& refs, const Box& cb, const Split& s, Refs* left, Refs* right) const {
        const double scale = centroid_scale(cb, s.axis);
        auto it = std::partition(refs.begin(), refs.end(),
                                 [&](int32_t r) { return centroid_bin(r, s.axis, cb, scale) <= s.split; });
        const int64_t mid = it - refs.begin();
        if (mid == 0 || mid == (int64_t)refs.size()) return median_halves(refs, left, right);
        left->assign(refs.begin(), it);
        right->assign(it, refs.end());
    }
    // spatial-split bins [*b0, *b1] that reference r's box spans: cells of width w from lo on axis ax
    void span_bins(int32_t r, int ax, double lo, double w, int* b0, int* b1) const {
        const Box& rb = tb[(size_t)r];
        *b0 = (int)(((double)rb.lo[ax] - lo) / w);
        *b1 = (int)(((double)rb.hi[ax] - lo) / w);
        *b0 = std::min(std::max(*b0, 0), knobs.bins - 1);
        *b1 = std::min(std::max(*b1, *b0), knobs.bins - 1);
    }
    double slab_width(const Box& b, int ax) const { return ((double)b.hi[ax] - b.lo[ax]) / knobs.bins; }
    // binned SAH spatial split of node box b; the sides' boxes are the search's upper bounds
    Split spatial_split(const Refs& refs, const Box& b) const {
        Split best;
        for (int ax = 0; ax < 3; ++ax) {
            const double lo = b.lo[ax];
            if (!((double)b.hi[ax] - b.lo[ax] > 0.0)) continue;
            const double w = slab_width(b, ax);
            Box bb[kMaxBins];
            int64_t entry[kMaxBins] = {0}, exit_[kMaxBins] = {0};
            for (int32_t r : refs) {
                const Box& rb = tb[(size_t)r];
                int b0, b1;
                span_bins(r, ax, lo, w, &b0, &b1);
                entry[b0]++;
                exit_[b1]++;
                if (b0 == b1) {
                    bb[b0].grow(rb);
                    continue;
                }
                // the search bins the reference box cut by the bin's slab (an upper bound of the
                // clipped triangle's bounds, exact for axis-aligned faces); the split itself clips
                for (int c = b0; c <= b1; ++c) {
                    Box part = rb;
                    if (c > b0) part.lo[ax] = std::max(part.lo[ax], (float)(lo + w * c));
                    if (c < b1) part.hi[ax] = std::min(part.hi[ax], (float)(lo + w * (c + 1)));
                    bb[c].grow(part);
                }
            }
            sweep(ax, bb, entry, exit_, &best);
        }
        return best;
    }
    // classifies by the same bins as the search; a straddling reference is split in two (a new
    // reference is appended: tb / cen / ref_tri grow, so boxes are copied before) or moved whole
    void partition_spatial(const Refs& refs, const Box& b, const Split& s, Refs* left, Refs* right) {
        const int ax = s.axis;
        const double lo = b.lo[ax], w = slab_width(b, ax);
        const double plane = lo + w * (s.split + 1);
        Refs straddle;
        Box lb, rb_;
        for (int32_t r : refs) {
            int b0, b1;
            span_bins(r, ax, lo, w, &b0, &b1);
            if (b1 <= s.split) { left->push_back(r); lb.grow(tb[(size_t)r]); }
            else if (b0 > s.split) { right->push_back(r); rb_.grow(tb[(size_t)r]); }
            else straddle.push_back(r);
        }
        for (int32_t r : straddle) {
            Box pl, pr;
            const bool hl = clip_ref(r, -INFINITY, plane, ax, &pl), hr = clip_ref(r, plane, INFINITY, ax, &pr);
            if (!hr || (!hl && !hr)) { left->push_back(r); lb.grow(tb[(size_t)r]); continue; }
            if (!hl) { right->push_back(r); rb_.grow(tb[(size_t)r]); continue; }
            // reference unsplitting (Stich et al. 2009 §4.3): whole to one side when cheaper
            const double nl = (double)left->size() + 1, nr = (double)right->size() + 1;
            Box lsplit = lb, rsplit = rb_, lwhole = lb, rwhole = rb_;
            lsplit.grow(pl); rsplit.grow(pr);
            lwhole.grow(tb[(size_t)r]); rwhole.grow(tb[(size_t)r]);
            const double c_split = lsplit.area() * nl + rsplit.area() * nr;
            const double c_left = lwhole.area() * nl + rb_.area() * (nr - 1);
            const double c_right = lb.area() * (nl - 1) + rwhole.area() * nr;
            if ((int64_t)tb.size() >= ref_budget || (c_left <= c_split && c_left <= c_right)) {
                left->push_back(r); lb = lwhole;
            } else if (c_right <= c_split) {
                right->push_back(r); rb_ = rwhole;
            } else {
                const int32_t r2 = (int32_t)tb.size();
                tb[(size_t)r] = pl;
                set_centre(r);
                tb.push_back(pr);
                ref_tri.push_back(ref_tri[(size_t)r]);
                cen.resize(cen.size() + 3);
                set_centre(r2);
                left->push_back(r); lb = lsplit;
                right->push_back(r2); rb_ = rsplit;
            }
        }
        if (left->empty() || right->empty()) {   // degenerate plane: everything on one side
            Refs all(*left);
            all.insert(all.end(), right->begin(), right->end());
            median_halves(all, left, right);
        }
    }
    // the fall-back of every split that cannot separate its references: the range cut in half
    static void median_halves(const Refs& refs, Refs* left, Refs* right) {
        const int64_t mid = (int64_t)refs.size() / 2;
        left->assign(refs.begin(), refs.begin() + mid);
        right->assign(refs.begin() + mid, refs.end());
    }
    int32_t make_leaf(int32_t me, const Refs& refs) {
        nodes[me].first = (int64_t)order.size();
        nodes[me].count = (int32_t)refs.size();
        order.insert(order.end(), refs.begin(), refs.end());
        leaves++;
        return me;
    }

    int32_t build(Refs& refs, int depth) {
        const int64_t count = (int64_t)refs.size();
        const int32_t me = (int32_t)nodes.size();
        nodes.emplace_back();   // may move `nodes`: index, never hold a TNode&
        Box b, cb;
        for (int32_t r : refs) {
            b.grow(tb[(size_t)r]);
            cb.grow(&cen[3 * (size_t)r]);
        }
        nodes[me].box = b;
        max_depth = std::max(max_depth, depth);
        if (count <= max_leaf && (count <= knobs.leaf_min || depth > 32)) return make_leaf(me, refs);
        Refs left, right;
        if (depth >= 32) {
            // depth guard (bounds the traversal stack): object median on the widest centroid axis
            int ax = 0;
            for (int a = 1; a < 3; ++a)
                if (cb.hi[a] - cb.lo[a] > cb.hi[ax] - cb.lo[ax]) ax = a;
            std::nth_element(refs.begin(), refs.begin() + count / 2, refs.end(),
                             [&](int32_t a, int32_t c) { return cen[3 * (size_t)a + ax] < cen[3 * (size_t)c + ax]; });
            median_halves(refs, &left, &right);
        } else {
            const Split obj = object_split(refs, cb);
            // spatial split: only where the object split's children overlap, within the reference budget
            const bool try_spatial = knobs.sbvh && obj.axis >= 0 && (int64_t)tb.size() < ref_budget &&
                                     meet(obj.left, obj.right).area() > min_overlap;
            const Split spa = try_spatial ? spatial_split(refs, b) : Split();
            const bool spatial = spa.axis >= 0 && spa.cost < obj.cost;
            const double split_sah = spatial ? spa.cost : obj.cost;
            const double parent_area = b.area();
            const double leaf_cost = (double)count;
            const double split_cost = parent_area > 0.0 ? knobs.ct + split_sah / parent_area : DBL_MAX;
            if (count <= max_leaf && !(split_cost < leaf_cost)) return make_leaf(me, refs);
            if (spatial) {
                spatial_splits++;
                partition_spatial(refs, b, spa, &left, &right);
            } else if (obj.axis < 0) {
                median_halves(refs, &left, &right);   // all centroids coincide: split the range
            } else {
                partition_object(refs, cb, obj, &left, &right);
            }
        }
        Refs().swap(refs);   // released before recursing: bounds the peak memory of a 1 M-triangle build
        const int32_t l = build(left, depth + 1);
        const int32_t r = build(right, depth + 1);
        nodes[me].left = l;
        nodes[me].right = r;
        return me;
    }
};

// the nodes below `root`, children (left first) before their parent
void postorder(const std::vector<TNode>& nodes, int32_t root, std::vector<int32_t>* post) {
    post->clear();
    std::vector<std::pair<int32_t, bool>> st(1, {root, false});
    while (!st.empty()) {
        const auto [t, done] = st.back();
        st.pop_back();
        if (done || nodes[t].count > 0) { post->push_back(t); continue; }
        st.push_back({t, true});
        st.push_back({nodes[t].right, false});
        st.push_back({nodes[t].left, false});
    }
}

// Treelet restructuring (Karras & Aila 2013, "Fast Parallel Construction of High-Quality Bounding
// Volume Hierarchies" §4): bottom-up, each inner node and its descendants down to 7 subtrees (the
// largest-area subtree expanded first) form a treelet whose binary topology over those 7 subtrees
// is replaced by the SAH-optimal one (a dynamic program over the 127 subsets), reusing the
// treelet's inner nodes.  Leaves and the references they hold are unchanged, so the leaf order
// and the triangle records stay valid; only inner boxes and child links move.  SAH cost of a
// subtree: leaf area x references, inner node ct x area + its children's costs.
void restructure_treelets(std::vector<TNode>& nodes, int32_t root, double ct, int passes, bool verbose) {
    constexpr int kT = 7;
    std::vector<double> cost(nodes.size(), 0.0);
    std::vector<int32_t> post;
    double box_a[1 << kT];
    Box box_m[1 << kT];
    double copt[1 << kT];
    int part[1 << kT];
    for (int pass = 0; pass < passes; ++pass) {
        postorder(nodes, root, &post);
        int64_t changed = 0;
        for (int32_t t : post) {
            TNode& nd = nodes[t];
            if (nd.count > 0) { cost[t] = nd.box.area() * nd.count; continue; }
            int32_t lv[kT] = {nd.left, nd.right};
            int32_t inner[kT];
            int nl = 2, ni = 0;
            double old = ct * nd.box.area();
            while (nl < kT) {
                int j = -1;
                double best_a = -1.0;
                for (int i = 0; i < nl; ++i)
                    if (nodes[lv[i]].count == 0 && nodes[lv[i]].box.area() > best_a) { best_a = nodes[lv[i]].box.area(); j = i; }
                if (j < 0) break;
                const int32_t x = lv[j];
                inner[ni++] = x;
                old += ct * best_a;
                lv[j] = nodes[x].left;
                lv[nl++] = nodes[x].right;
            }
            for (int i = 0; i < nl; ++i) old += cost[lv[i]];
            if (nl < 3) { cost[t] = old; continue; }
            const int full = (1 << nl) - 1;
            for (int m = 1; m <= full; ++m) {
                const int low = m & -m;
                if (m == low) {
                    const int i = __builtin_ctz((unsigned)m);
                    box_m[m] = nodes[lv[i]].box;
                    copt[m] = cost[lv[i]];
                    continue;
                }
                box_m[m] = box_m[m ^ low];
                box_m[m].grow(box_m[low]);
                box_a[m] = box_m[m].area();
                double best = DBL_MAX;
                int bp = 0;
                // partitions {sub, m ^ sub} with the lowest subtree in sub (each split once)
                for (int sub = (m - 1) & m; sub; sub = (sub - 1) & m) {
                    if (!(sub & low)) continue;
                    const double c = copt[sub] + copt[m ^ sub];
                    if (c < best) { best = c; bp = sub; }
                }
                copt[m] = ct * box_a[m] + best;
                part[m] = bp;
            }
            if (!(copt[full] < old * (1.0 - 1e-12))) { cost[t] = old; continue; }
            // rebuild the treelet below t with the optimal splits, reusing its inner nodes
            int used = 0;
            std::vector<std::pair<int32_t, int>> todo{{t, full}};
            while (!todo.empty()) {
                const auto [id, m] = todo.back();
                todo.pop_back();
                const int a = part[m], b = m ^ part[m];
                int32_t kids[2];
                const int ms[2] = {a, b};
                for (int s = 0; s < 2; ++s) {
                    if ((ms[s] & (ms[s] - 1)) == 0) {
                        kids[s] = lv[__builtin_ctz((unsigned)ms[s])];
                    } else {
                        const int32_t nid = inner[used++];
                        nodes[nid].box = box_m[ms[s]];
                        nodes[nid].count = 0;
                        cost[nid] = copt[ms[s]];
                        todo.push_back({nid, ms[s]});
                        kids[s] = nid;
                    }
                }
                nodes[id].left = kids[0];
                nodes[id].right = kids[1];
            }
            cost[t] = copt[full];
            ++changed;
        }
        if (verbose)
            std::fprintf(stderr, "prt_bvh: treelet pass %d: %lld treelets restructured, SAH %.3f\n", pass,
                         (long long)changed, nodes[root].box.area() > 0 ? cost[root] / nodes[root].box.area() : 0.0);
        if (!changed) break;
    }
}

// depth of the deepest node below `root` (root = 0), as Builder::build counts it
int32_t tree_depth(const std::vector<TNode>& nodes, int32_t root) {
    int32_t d = 0;
    std::vector<std::pair<int32_t, int32_t>> st{{root, 0}};
    while (!st.empty()) {
        const auto [t, k] = st.back();
        st.pop_back();
        d = std::max(d, k);
        if (nodes[t].count == 0) { st.push_back({nodes[t].left, k + 1}); st.push_back({nodes[t].right, k + 1}); }
    }
    return d;
}

// The build's references (B->tb / ref_tri / cen): one per triangle, several (early split clipping) for
// triangles whose box area exceeds esc_beta x the mean (0 = off; at most 2 n_tri + 4096 in all).  Also
// the scene's box.
bool make_references(const float* tri_v, int64_t n_tri, double esc_beta, Builder* B, Box* scene, std::string* err) {
    std::vector<Box> tri_box((size_t)n_tri);
    double mean_area = 0.0;
    for (int64_t i = 0; i < n_tri; ++i) {
        const float* t = tri_v + 9 * i;
        Box b;
        b.grow(t); b.grow(t + 3); b.grow(t + 6);
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(t[k])) { *err = "non-finite vertex in triangle " + std::to_string(i); return false; }
        tri_box[(size_t)i] = b;
        mean_area += b.area();
        scene->grow(b);
    }
    mean_area /= (double)std::max<int64_t>(n_tri, 1);
    B->ref_tri.reserve((size_t)n_tri);
    // the cap stays below the 2^27 references the leaf encoding addresses: past it every further
    // triangle keeps one reference (a scene with < 2^27 triangles always builds)
    const int64_t ref_cap = std::min<int64_t>(2 * n_tri + 4096, ((int64_t)1 << 27) - 1);
    std::vector<RefBox> pieces;
    for (int64_t i = 0; i < n_tri; ++i) {
        const Box& b = tri_box[(size_t)i];
        pieces.clear();
        // mean_area > 0: a scene of degenerate boxes (area 0) would split every other triangle
        // to the maximum depth against a zero threshold
        if (esc_beta > 0.0 && mean_area > 0.0 && b.area() > esc_beta * mean_area && (int64_t)B->tb.size() < ref_cap) {
            RefBox cell;
            for (int k = 0; k < 3; ++k) { cell.lo[k] = b.lo[k]; cell.hi[k] = b.hi[k]; }
            split_refs(tri_v + 9 * i, cell, esc_beta * mean_area, 0, &pieces);
        }
        // one triangle yields up to 2^12 pieces: past the remaining budget it keeps one reference
        if (pieces.size() <= 1 || (int64_t)(B->tb.size() + pieces.size() + (size_t)(n_tri - i - 1)) > ref_cap) {
            B->tb.push_back(b);
            B->ref_tri.push_back((int32_t)i);
        } else {
            for (const RefBox& r : pieces) {
                B->tb.push_back(outward_f32(r, b));
                B->ref_tri.push_back((int32_t)i);
            }
        }
    }
    if ((int64_t)B->tb.size() >= ((int64_t)1 << 27)) { *err = "too many BVH references (< 2^27)"; return false; }
    B->cen.resize(B->tb.size() * 3);
    for (size_t r = 0; r < B->tb.size(); ++r) B->set_centre((int32_t)r);
    return true;
}

// child box `side` of a 64-B node record, padded; an invalid box is inverted (missed by every ray)
void put_box(float* f, int side, const Box& bx, bool valid, float pad) {
    for (int k = 0; k < 3; ++k) {
        f[6 * side + 2 * k] = valid ? bx.lo[k] - pad : INFINITY;
        f[6 * side + 2 * k + 1] = valid ? bx.hi[k] + pad : -INFINITY;
    }
}

// The temporary tree as the flat arrays of BvhHost: inner nodes numbered in DFS preorder, leaves as
// child references into the leaf order, which is also the order of the triangle records.
void flatten(const Builder& B, int32_t root, float pad, BvhHost* out) {
    const int64_t n_ref = (int64_t)B.order.size();
    std::vector<int32_t> inner_id(B.nodes.size(), -1), preorder, stack;
    if (root >= 0 && B.nodes[root].count == 0) stack.push_back(root);
    while (!stack.empty()) {
        int32_t t = stack.back(); stack.pop_back();
        inner_id[t] = (int32_t)preorder.size();
        preorder.push_back(t);
        const TNode& nd = B.nodes[t];
        if (B.nodes[nd.right].count == 0) stack.push_back(nd.right);
        if (B.nodes[nd.left].count == 0) stack.push_back(nd.left);
    }
    auto child_ref = [&](int32_t t) -> int32_t {
        const TNode& c = B.nodes[t];
        return c.count > 0 ? leaf_ref(c.first, c.count) : inner_id[t];
    };
    out->n_nodes = std::max<int64_t>((int64_t)preorder.size(), 1);
    out->nodes.assign((size_t)out->n_nodes * 16, 0.0f);
    if (preorder.empty()) {
        // empty scene or a single leaf: one inner node, left = leaf (if any), right = empty
        float* f = out->nodes.data();
        Box empty;
        if (root >= 0) put_box(f, 0, B.nodes[root].box, true, pad); else put_box(f, 0, empty, false, pad);
        put_box(f, 1, empty, false, pad);
        f[12] = f[13] = bits<float>(root >= 0 ? leaf_ref(0, (int)n_ref) : leaf_ref(0, 1));
    }
    for (int32_t t : preorder) {
        float* f = out->nodes.data() + (size_t)inner_id[t] * 16;
        const TNode& nd = B.nodes[t];
        put_box(f, 0, B.nodes[nd.left].box, true, pad);
        put_box(f, 1, B.nodes[nd.right].box, true, pad);
        f[12] = bits<float>(child_ref(nd.left));
        f[13] = bits<float>(child_ref(nd.right));
    }
    out->order.resize((size_t)n_ref);
    out->tris.assign((size_t)n_ref * 12, 0.0f);
    for (int64_t s = 0; s < n_ref; ++s) {
        const int32_t o = out->order[(size_t)s] = B.ref_tri[(size_t)B.order[(size_t)s]];
        const float* t = B.tv + 9 * (int64_t)o;
        float* d = out->tris.data() + 12 * s;
        for (int k = 0; k < 3; ++k) {
            d[k] = t[k];
            d[4 + k] = t[3 + k] - t[k];   // e1 = v1 - v0 in f32 (bit-identical to on-the-fly)
            d[8 + k] = t[6 + k] - t[k];   // e2 = v2 - v0
        }
        d[3] = bits<float>(o);
    }
}

// counts, depth and the tree's SAH cost: leaf area x references, inner node area x 1, over the root's area
void statistics(const Builder& B, int32_t root, BvhHost* out) {
    out->n_refs = (int64_t)B.order.size();
    out->depth = out->n_refs > 0 ? std::max(1, B.max_depth) : 1;
    out->n_leaves = B.leaves;
    out->n_spatial = B.spatial_splits;
    out->sah_cost = 0.0;
    if (root >= 0 && B.nodes[root].box.area() > 0.0) {
        const double ra = B.nodes[root].box.area();
        for (const TNode& nd : B.nodes) out->sah_cost += nd.box.area() / ra * (nd.count > 0 ? (double)nd.count : 1.0);
    }
}

}  // namespace

// Padding: ~8 ulps of the largest coordinate magnitude / extent.  Keeps the
// slab test conservative against Moller-Trumbore accepting hit points that
// lie a rounding error outside the triangle (axis-aligned Cornell edges).
float bvh_pad(const float* tri_v, int64_t n_tri) {
    Box scene;
    float max_abs = 0.0f;
    for (int64_t i = 0; i < 3 * n_tri; ++i) {
        scene.grow(tri_v + 3 * i);
        for (int k = 0; k < 3; ++k) max_abs = std::max(max_abs, std::fabs(tri_v[3 * i + k]));
    }
    const float extent = scene.valid() ? std::max({scene.hi[0] - scene.lo[0], scene.hi[1] - scene.lo[1], scene.hi[2] - scene.lo[2]}) : 0.0f;
    return std::max(max_abs, extent) * 1e-6f + 1e-30f;
}

bool build_bvh(const float* tri_v, int64_t n_tri, int max_leaf, BvhHost* out, std::string* err) {
    if (max_leaf < 1 || max_leaf > kMaxLeaf) { *err = "max_leaf must be in [1, 8]"; return false; }
    if (n_tri < 0 || n_tri >= ((int64_t)1 << 27)) { *err = "triangle count out of range (< 2^27)"; return false; }
    Builder B;
    B.tv = tri_v; B.max_leaf = max_leaf;
    B.knobs = read_bvh_knobs(n_tri, max_leaf);
    Box scene;
    if (!make_references(tri_v, n_tri, B.knobs.esc_beta, &B, &scene, err)) return false;
    const int64_t n_ref0 = (int64_t)B.tb.size();
    // spatial splits add references up to the budget, below the 2^27 the leaf encoding addresses
    B.ref_budget = std::min<int64_t>((int64_t)((double)n_ref0 * B.knobs.budget), ((int64_t)1 << 27) - 1);
    int32_t root = -1;
    if (n_ref0 > 0) {
        std::vector<int32_t> all((size_t)n_ref0);
        for (int64_t i = 0; i < n_ref0; ++i) all[(size_t)i] = (int32_t)i;
        B.nodes.reserve((size_t)(2 * n_ref0 / std::max(1, max_leaf / 2) + 8));
        if (scene.valid()) B.min_overlap = B.knobs.alpha * scene.area();
        root = B.build(all, 0);
        if (B.knobs.treelet > 0 && B.nodes[root].count == 0) {
            restructure_treelets(B.nodes, root, B.knobs.ct, B.knobs.treelet, B.knobs.verbose);
            B.max_depth = tree_depth(B.nodes, root);
        }
    }
    // every reference sits in exactly one leaf: the leaf order is the triangle records' order
    const int64_t n_ref = (int64_t)B.order.size();
    if (n_ref != (int64_t)B.tb.size()) { *err = "internal: BVH references lost in the build"; return false; }
    out->pad = bvh_pad(tri_v, n_tri);
    flatten(B, root, out->pad, out);
    statistics(B, root, out);
    if (B.knobs.verbose)
        std::fprintf(stderr, "prt_bvh: %lld triangles, %lld references (%lld before spatial splits), %lld spatial "
                             "splits, %lld leaves, depth %d, SAH %.3f\n", (long long)n_tri, (long long)n_ref,
                     (long long)n_ref0, (long long)B.spatial_splits, (long long)B.leaves, (int)out->depth, out->sah_cost);
    return true;
}

}  // namespace prt

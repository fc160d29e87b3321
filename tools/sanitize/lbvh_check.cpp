// lbvh_check — host driver for the sanitizer build of the host bookkeeping of prt_scene_rebuild
// (pyrenderer_amd/csrc/prt_plan.cpp: lbvh_scratch, lbvh_node_capacity, LbvhLevels, iota_list, wide_stack_need;
// DESIGN.md §14).  tools/sanitize/Makefile compiles it with prt_plan.cpp under g++ -fsanitize=address,undefined,
// every finding fatal; tests/test_lbvh_abi.py runs it.
//
//   lbvh_check <n_slots> <seed> [distinct codes, default 0 = as many as slots allow]
// draws sorted 30-bit codes (with duplicates), makes the keys code << 32 | slot, and walks the device build's
// stages on the CPU with the library's own bookkeeping: the per-node split search of prt_lbvh.hip restated
// here gives, for every inner node, the split that a bisection of its range gives; the four- and eight-wide
// trees emitted level by level stay within lbvh_node_capacity and the work arrays of lbvh_scratch, every slot
// sits in exactly one leaf of at most max_leaf, wide_levels accepts the records and finds LbvhLevels'
// offsets, and the stack need is that of a depth-first walk.  Prints one JSON line; exit status 0 unless the
// command line is unusable.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "prt_internal.h"
#include "prt_plan.h"

namespace {

using Keys = std::vector<uint64_t>;

int delta(const Keys& k, int64_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)k.size()) return -1;
    return __builtin_clzll(k[(size_t)i] ^ k[(size_t)j]);
}

// lbvh_topology_kernel's search, statement for statement
int32_t node_split(const Keys& k, int64_t i) {
    const int64_t d = delta(k, i, i + 1) > delta(k, i, i - 1) ? 1 : -1;
    const int dmin = delta(k, i, i - d);
    int64_t lmax = 2;
    while (delta(k, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(k, i, i + (l + t) * d) > dmin) l += t;
    const int dnode = delta(k, i, i + l * d);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta(k, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    return (int32_t)(i + s * d + (d < 0 ? -1 : 0));
}

// the split of the range [a, b] by bisection: the last key sharing key a's bits above the highest differing one
int32_t range_split(const Keys& k, int64_t a, int64_t b) {
    const int bit = 63 - __builtin_clzll(k[(size_t)a] ^ k[(size_t)b]);
    int64_t lo = a, hi = b;
    while (lo < hi) {
        const int64_t m = (lo + hi + 1) / 2;
        if ((k[(size_t)m] >> bit) == (k[(size_t)a] >> bit)) lo = m; else hi = m - 1;
    }
    return (int32_t)lo;
}

struct Item { int32_t a, b, idx, anc; };

std::vector<Item> children(const Item& it, const std::vector<int32_t>& split, int max_leaf, int width) {
    std::vector<Item> ch;
    if (it.b < it.a) return ch;
    ch.push_back(it);
    for (int round = 1; round < width; round *= 2) {
        std::vector<Item> next;
        for (const Item& c : ch) {
            if (c.b - c.a + 1 <= max_leaf) { next.push_back(c); continue; }
            const int32_t s = split[(size_t)c.idx];
            next.push_back(Item{c.a, s, s, 0});
            next.push_back(Item{s + 1, c.b, s + 1, 0});
        }
        ch.swap(next);
    }
    return ch;
}

int walk_need(const std::vector<float>& nodes, int width, int64_t stride) {
    int most = 0;
    std::vector<std::pair<int32_t, int>> stack{{0, 0}};
    while (!stack.empty()) {
        const auto [i, held] = stack.back();
        stack.pop_back();
        most = std::max(most, held);
        int live = 0;
        int32_t refs[8];
        for (int k = 0; k < width; ++k) {
            std::memcpy(&refs[k], nodes.data() + (size_t)i * stride + 6 * width + k, 4);
            live += refs[k] != 0x7FFFFFFF;
        }
        for (int k = 0; k < width; ++k)
            if (refs[k] >= 0 && refs[k] != 0x7FFFFFFF) stack.push_back({refs[k], held + live - 1});
    }
    return prt::wide_stack_need(most, width);
}

// one width: failures, with the tree's nodes, levels and need out
int emit(const Keys& keys, const std::vector<int32_t>& split, int max_leaf, int width, int64_t* n_nodes, int* levels,
         int* need) {
    const int64_t n = (int64_t)keys.size(), cap = prt::lbvh_node_capacity(n), widest = n / 2 + 1;
    const prt::LbvhScratch z = prt::lbvh_scratch(n);
    const int64_t stride = width == 8 ? prt::kNode8F4 * 4 : prt::kNode4F4 * 4;
    int bad = 0;
    std::vector<Item> items((size_t)(z.item / sizeof(Item)));
    std::vector<int32_t> child0(z.word / 4), cnt(z.count / 4);
    bad += (int64_t)items.size() < cap;
    items[0] = Item{0, (int32_t)(n - 1), 0, 0};
    prt::LbvhLevels lv;
    bad += !lv.push(1, cap, widest);
    int max_anc = 0;
    for (;;) {
        const int64_t base = lv.off[(size_t)lv.depth()], count = lv.n_nodes() - base;
        int64_t at = lv.n_nodes();
        bad += (size_t)count + 1 > cnt.size();
        for (int64_t j = 0; j < count; ++j) {
            const Item it = items[(size_t)(base + j)];
            const std::vector<Item> ch = children(it, split, max_leaf, width);
            child0[(size_t)(base + j)] = (int32_t)at;
            int inner = 0;
            for (const Item& c : ch)
                if (c.b - c.a + 1 > max_leaf) {
                    items.at((size_t)at++) = Item{c.a, c.b, c.idx, it.anc + (int32_t)ch.size() - 1};
                    ++inner;
                }
            cnt[(size_t)j] = inner;
            max_anc = std::max(max_anc, it.anc);
        }
        const int64_t next = at - lv.n_nodes();
        if (next == 0) break;
        if (!lv.push(next, cap, widest)) { ++bad; break; }
    }
    bad += lv.push(-1, cap, widest) || lv.push(cap + 1, cap, widest + cap);   // refused: negative, beyond capacity
    std::vector<float> nodes((size_t)(lv.n_nodes() * stride), 0.0f);
    std::vector<int> seen((size_t)n, 0);
    for (int64_t i = 0; i < lv.n_nodes(); ++i) {
        const std::vector<Item> ch = children(items[(size_t)i], split, max_leaf, width);
        int32_t next = child0[(size_t)i];
        for (int k = 0; k < width; ++k) {
            int32_t ref = 0x7FFFFFFF;
            if (k < (int)ch.size()) {
                const int count = ch[(size_t)k].b - ch[(size_t)k].a + 1;
                if (count > max_leaf) {
                    ref = next++;
                } else {
                    ref = prt::leaf_ref(ch[(size_t)k].a, count);
                    bad += prt::leaf_first(ref) != ch[(size_t)k].a || prt::leaf_count(ref) != count;
                    for (int t = 0; t < count; ++t) ++seen[(size_t)(ch[(size_t)k].a + t)];
                }
            }
            std::memcpy(nodes.data() + (size_t)i * stride + 6 * width + k, &ref, 4);
        }
    }
    for (int v : seen) bad += v != 1;
    std::vector<int32_t> list;
    std::vector<int64_t> off;
    bad += !prt::wide_levels(nodes.data(), lv.n_nodes(), width, &list, &off);
    bad += off != lv.off || list != prt::iota_list(lv.n_nodes());
    *need = prt::wide_stack_need(max_anc, width);
    bad += *need != walk_need(nodes, width, stride);
    *n_nodes = lv.n_nodes();
    *levels = lv.depth() + 1;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: lbvh_check <n_slots> <seed> [distinct codes]\n"); return 2; }
    const int64_t n = std::atoll(argv[1]);
    const unsigned seed = (unsigned)std::atoi(argv[2]);
    const int64_t distinct = argc > 3 ? std::atoll(argv[3]) : 0;
    if (n < 0 || n >= prt::kLbvhMaxSlots) { std::fprintf(stderr, "n_slots out of range\n"); return 2; }
    std::mt19937 rng(seed);
    std::vector<uint32_t> codes((size_t)n);
    for (auto& c : codes) c = distinct > 0 ? (uint32_t)(rng() % (uint64_t)distinct) * 7919u & 0x3FFFFFFFu : rng() & 0x3FFFFFFFu;
    std::sort(codes.begin(), codes.end());
    Keys keys((size_t)n);
    for (int64_t s = 0; s < n; ++s) keys[(size_t)s] = ((uint64_t)codes[(size_t)s] << 32) | (uint64_t)s;
    const int max_leaf = 4;
    int failures = 0;
    // stage 3: every inner node's split, and the range it belongs to, against the bisection
    std::vector<int32_t> split((size_t)std::max<int64_t>(n - 1, 0), -1);
    for (int64_t i = 0; i + 1 < n; ++i) split[(size_t)i] = node_split(keys, i);
    int64_t ranges = 0;
    if (n >= 2) {
        std::vector<Item> work{Item{0, (int32_t)(n - 1), 0, 0}};
        while (!work.empty()) {
            const Item it = work.back();
            work.pop_back();
            ++ranges;
            const int32_t s = split[(size_t)it.idx];
            failures += s != range_split(keys, it.a, it.b);
            if (s < it.a || s >= it.b) { ++failures; continue; }
            if (s > it.a) work.push_back(Item{it.a, s, s, 0});
            if (s + 1 < it.b) work.push_back(Item{s + 1, it.b, s + 1, 0});
        }
        failures += ranges != n - 1;     // every inner node is reached exactly once
    }
    int64_t nodes4 = 0, nodes8 = 0;
    int levels4 = 0, levels8 = 0, need4 = 0, need8 = 0;
    failures += emit(keys, split, max_leaf, 4, &nodes4, &levels4, &need4);
    failures += emit(keys, split, max_leaf, 8, &nodes8, &levels8, &need8);
    const prt::LbvhScratch z = prt::lbvh_scratch(n);
    failures += z.cen < 12 * (size_t)n || z.word < 4 * (size_t)n || z.key < 8 * (size_t)n;
    std::printf("{\"slots\": %lld, \"failures\": %d, \"inner\": %lld, \"nodes4\": %lld, \"levels4\": %d, \"need4\": %d, "
                "\"nodes8\": %lld, \"levels8\": %d, \"need8\": %d}\n",
                (long long)n, failures, (long long)ranges, (long long)nodes4, levels4, need4, (long long)nodes8, levels8,
                need8);
    return 0;
}

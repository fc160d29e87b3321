// refit_check — host driver for the sanitizer build of what prt_scene_update does on the host before it
// touches a device (pyrenderer_amd/csrc/prt_plan.cpp: validate_update, wide_levels; prt_bvh.cpp: bvh_pad), on
// trees of the library's own builder.  tools/sanitize/Makefile compiles it with the builder units under
// g++ -fsanitize=address,undefined, every finding fatal; tests/test_refit_abi.py runs it.
//
//   refit_check <n_tri> <seed>
// builds a random soup, collapses it to both widths and checks: every node is listed in exactly one level,
// a child sits one level below its parent, the offsets cover the list; a tree with a child numbered at or
// below its parent is refused; the pad rule gives the builder's pad; the update checks accept the soup and
// refuse a NaN vertex, an infinite normal, a zero radius, a NaN centre and NULL arrays.
// Prints one JSON line; exit status 0 unless the command line is unusable.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "prt_internal.h"
#include "prt_plan.h"

namespace {

int check_levels(const std::vector<float>& nodes, int64_t n_nodes, int width, int64_t* n_levels) {
    std::vector<int32_t> list;
    std::vector<int64_t> off;
    if (!prt::wide_levels(nodes.data(), n_nodes, width, &list, &off)) return 1;
    int bad = 0;
    const int64_t stride = width == 8 ? prt::kNode8F4 * 4 : prt::kNode4F4 * 4;
    std::vector<int32_t> level((size_t)n_nodes, -1);
    bad += off.empty() || off.front() != 0 || off.back() != n_nodes || (int64_t)list.size() != n_nodes;
    for (size_t l = 0; l + 1 < off.size(); ++l) {
        bad += off[l + 1] <= off[l];
        for (int64_t k = off[l]; k < off[l + 1]; ++k) {
            bad += level[(size_t)list[(size_t)k]] != -1;
            level[(size_t)list[(size_t)k]] = (int32_t)l;
        }
    }
    bad += n_nodes > 0 && level[0] != 0;
    for (int64_t i = 0; i < n_nodes; ++i)
        for (int k = 0; k < width; ++k) {
            int32_t ref;
            std::memcpy(&ref, nodes.data() + i * stride + 6 * width + k, 4);
            if (ref >= 0 && ref != 0x7FFFFFFF) bad += level[(size_t)ref] != level[(size_t)i] + 1;
        }
    // a child numbered at its parent: refused
    std::vector<float> broken = nodes;
    bool probed = false;
    for (int64_t i = 0; i < n_nodes && !probed; ++i)
        for (int k = 0; k < width; ++k) {
            int32_t ref;
            std::memcpy(&ref, broken.data() + i * stride + 6 * width + k, 4);
            if (ref >= 0 && ref != 0x7FFFFFFF) {
                const int32_t self = (int32_t)i;
                std::memcpy(broken.data() + i * stride + 6 * width + k, &self, 4);
                bad += prt::wide_levels(broken.data(), n_nodes, width, &list, &off);
                probed = true;   // once
                break;
            }
        }
    *n_levels = (int64_t)off.size() - 1;
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: refit_check <n_tri> <seed>\n");
        return 2;
    }
    const int64_t n = std::atoll(argv[1]);
    std::mt19937 rng((unsigned)std::atoi(argv[2]));
    std::uniform_real_distribution<float> pos(-1.0f, 1.0f), off(-0.05f, 0.05f);
    std::vector<float> tv((size_t)n * 9), tn((size_t)n * 3, 0.0f), sph = {0.0f, 0.5f, 0.0f, 0.25f};
    for (int64_t i = 0; i < n; ++i) {
        const float c[3] = {pos(rng), pos(rng), pos(rng)};
        for (int k = 0; k < 9; ++k) tv[(size_t)(9 * i + k)] = c[k % 3] + off(rng);
        tn[(size_t)(3 * i + 1)] = 1.0f;
    }
    int failures = 0;
    prt::BvhHost bvh;
    std::string err;
    if (!prt::build_bvh(tv.data(), n, 4, &bvh, &err)) {
        std::printf("{\"failures\": 1, \"error\": \"%s\"}\n", err.c_str());
        return 0;
    }
    failures += prt::bvh_pad(tv.data(), n) != bvh.pad;
    prt::Bvh4Host b4;
    prt::Bvh8Host b8;
    prt::collapse_bvh4(bvh, &b4);
    prt::collapse_bvh8(bvh, &b8);
    int64_t levels4 = 0, levels8 = 0;
    failures += check_levels(b4.nodes, b4.n_nodes, 4, &levels4);
    failures += check_levels(b8.nodes, b8.n_nodes, 8, &levels8);

    failures += !prt::validate_update(tv.data(), tn.data(), n, sph.data(), 1, &err);
    failures += !prt::validate_update(tv.data(), tn.data(), n, nullptr, 0, &err);
    int refused = 0;
    if (n > 0) {
        std::vector<float> v = tv, nn = tn;
        v[v.size() / 2] = NAN;
        refused += !prt::validate_update(v.data(), tn.data(), n, nullptr, 0, &err);
        nn.back() = INFINITY;
        refused += !prt::validate_update(tv.data(), nn.data(), n, nullptr, 0, &err);
        refused += !prt::validate_update(nullptr, tn.data(), n, nullptr, 0, &err);
        refused += !prt::validate_update(tv.data(), nullptr, n, nullptr, 0, &err);
    } else {
        refused += 4;
    }
    std::vector<float> s0 = sph, s1 = sph;
    s0[3] = 0.0f;
    s1[1] = NAN;
    refused += !prt::validate_update(tv.data(), tn.data(), n, s0.data(), 1, &err);
    refused += !prt::validate_update(tv.data(), tn.data(), n, s1.data(), 1, &err);
    refused += !prt::validate_update(tv.data(), tn.data(), n, nullptr, 1, &err);
    failures += refused != 7;
    std::printf("{\"failures\": %d, \"triangles\": %lld, \"references\": %lld, \"nodes4\": %lld, \"levels4\": %lld, "
                "\"nodes8\": %lld, \"levels8\": %lld, \"refused\": %d}\n", failures, (long long)n,
                (long long)bvh.order.size(), (long long)b4.n_nodes, (long long)levels4, (long long)b8.n_nodes,
                (long long)levels8, refused);
    return 0;
}

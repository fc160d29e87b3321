// host_check — host driver for the sanitizer build of libprt's GPU-free host arithmetic
// (pyrenderer_amd/csrc/prt_plan.cpp: standard library + prt_internal.h, prt_lds_layout.h and
// prt_variant_table.h only).  tools/sanitize/Makefile compiles both with g++ -fsanitize=address,undefined,float-cast-overflow, every finding fatal;
// tests/test_host_plan.py runs the modes below and checks the printed values against numpy.
//
//   host_check origins <tiles_x> <tw> <th> <id>...          packed origins of tile ids
//   host_check window <W> <x0> <y0> <w> <h> <tw> <th>       tile ids of a window
//   host_check in_frame <W> <H> <tw> <th> <id>...           per slot of those tiles: 1 inside the frame
//   host_check latin_stride <lo> <hi>                       latin_stride(n) for n = lo..hi
//   host_check latin <W> <H> <tile> <n_ranks>               per-rank tile ids
//   host_check chunks (<T> <n_slots> <bytes> <budget>)...   [chunk, launches] per quadruple
//   host_check frames <spp> <n_frames> <chunk>              [s0, n, f0, f1] of every launch of chunk samples
//   host_check camera <cam.f32>                             cam_fast and the bits of cam_o / cam_k
//   host_check env <NAME> <lo> <hi> <fallback>              env_int, and spill_lds_entries of it
//   host_check layout (<n_node_f4> <n_tri_f4> <n_tri> <n_mat> <n_lt> <n_light> <stack>)...
//       per size tuple: the float4 offsets of trace_lds and pool_lds in region order, their totals in
//       bytes, lds_scene_bytes, and trace_smem_bytes(stack, var, sizes) for var = 0 .. kVarLast + 1
//   host_check variant (<n_node_f4> <n_tri_f4> <n_tri> <n_mat> <n_lt> <n_light> <need4> <stack4>)...
//       per tuple: lds_fits, and choose_variant without and with the MIS estimator
//   host_check width (<n_node_f4> <n_tri_f4> <n_tri> <n_mat> <n_lt> <n_light> <stack> <width> <need8> <knob>)...
//       per tuple: lds_width of those sizes (the scene's with its BVH8), need8 and PRT_LDS_WIDTH = knob
//   host_check scene <dir> <n_tri> <n_sph> <n_mat> <n_light>
//       reads <dir>/{tri_v,tri_n,sph,mat}.f32 and {tri_mat,sph_mat,light_tri,light_off}.i32 (raw, as
//       numpy.tofile writes them; a missing file is a NULL argument), validates, and when valid packs
//       and writes <dir>/{tri_nm,tri_frame,light_v}.f32
// Prints one JSON line; exit status 0 unless the command line is unusable.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prt_plan.h"

namespace {

template <class T>
bool read_raw(const std::string& path, std::vector<T>* out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out->resize((size_t)bytes / sizeof(T) + 1);   // + 1: data() is non-null for an empty file too
    const size_t got = std::fread(out->data(), sizeof(T), out->size() - 1, f);
    std::fclose(f);
    return got == out->size() - 1;
}

void write_raw(const std::string& path, const std::vector<float>& v) {
    if (FILE* f = std::fopen(path.c_str(), "wb")) {
        std::fwrite(v.data(), sizeof(float), v.size(), f);
        std::fclose(f);
    }
}

template <class V>
void print_list(const V& v) {
    std::printf("[");
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
    std::printf("]");
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

std::vector<int32_t> int_args(int argc, char** argv, int first) {
    std::vector<int32_t> v;
    for (int i = first; i < argc; ++i) v.push_back((int32_t)std::atoi(argv[i]));
    return v;
}

int scene_mode(const std::string& dir, long long n_tri, long long n_sph, int n_mat, int n_light) {
    std::vector<float> tri_v, tri_n, sph, mat;
    std::vector<int32_t> tri_mat, sph_mat, light_tri, light_off;
    prt::SceneArgs a{};
    if (read_raw(dir + "/tri_v.f32", &tri_v)) a.tri_v = tri_v.data();
    if (read_raw(dir + "/tri_n.f32", &tri_n)) a.tri_n = tri_n.data();
    if (read_raw(dir + "/tri_mat.i32", &tri_mat)) a.tri_mat = tri_mat.data();
    if (read_raw(dir + "/sph.f32", &sph)) a.sph = sph.data();
    if (read_raw(dir + "/sph_mat.i32", &sph_mat)) a.sph_mat = sph_mat.data();
    if (read_raw(dir + "/mat.f32", &mat)) a.mat = mat.data();
    if (read_raw(dir + "/light_tri.i32", &light_tri)) a.light_tri = light_tri.data();
    if (read_raw(dir + "/light_off.i32", &light_off)) a.light_off = light_off.data();
    a.n_tri = n_tri; a.n_sph = n_sph; a.n_mat = n_mat; a.n_light = n_light;
    std::string err;
    if (!prt::validate_scene(a, &err)) {
        std::printf("{\"error\": \"%s\"}\n", err.c_str());
        return 0;
    }
    prt::PackedScene pk;
    prt::pack_scene(a, &pk);
    write_raw(dir + "/tri_nm.f32", pk.tri_nm);
    write_raw(dir + "/tri_frame.f32", pk.tri_frame);
    write_raw(dir + "/light_v.f32", pk.light_v);
    std::printf("{\"error\": null, \"n_lt\": %d, \"plain\": %s, \"shade_fast\": %s}\n", pk.n_lt,
                pk.plain ? "true" : "false", pk.shade_fast ? "true" : "false");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    auto num = [&](int i) { return std::atoll(argv[i]); };
    if (mode == "origins" && argc >= 5) {
        const std::vector<int32_t> ids = int_args(argc, argv, 5);
        std::printf("{\"origins\": ");
        print_list(prt::tile_origins(ids.data(), (int64_t)ids.size(), (int)num(2), (int)num(3), (int)num(4)));
        std::printf("}\n");
    } else if (mode == "window" && argc == 9) {
        std::printf("{\"ids\": ");
        print_list(prt::window_tiles((int)num(2), (int)num(3), (int)num(4), (int)num(5), (int)num(6), (int)num(7),
                                     (int)num(8)));
        std::printf("}\n");
    } else if (mode == "in_frame" && argc >= 6) {
        const int W = (int)num(2), H = (int)num(3), tw = (int)num(4), th = (int)num(5);
        const std::vector<int32_t> ids = int_args(argc, argv, 6);
        const std::vector<uint32_t> xy = prt::tile_origins(ids.data(), (int64_t)ids.size(), (W + tw - 1) / tw, tw, th);
        std::vector<int> in;
        for (int64_t slot = 0; slot < (int64_t)ids.size() * tw * th; ++slot)
            in.push_back(prt::slot_in_frame(xy, slot, tw, th, W, H) ? 1 : 0);
        std::printf("{\"in_frame\": ");
        print_list(in);
        std::printf("}\n");
    } else if (mode == "latin_stride" && argc == 4) {
        std::vector<int> s;
        for (int n = (int)num(2); n <= (int)num(3); ++n) s.push_back(prt::latin_stride(n));
        std::printf("{\"strides\": ");
        print_list(s);
        std::printf("}\n");
    } else if (mode == "latin" && argc == 6) {
        const auto ids = prt::latin_tile_ids((int)num(2), (int)num(3), (int)num(4), (int)num(5));
        std::printf("{\"ids\": [");
        for (size_t r = 0; r < ids.size(); ++r) {
            if (r) std::printf(", ");
            print_list(ids[r]);
        }
        std::printf("]}\n");
    } else if (mode == "chunks" && argc >= 6 && (argc - 2) % 4 == 0) {
        std::printf("{\"plans\": [");
        for (int i = 2; i < argc; i += 4) {
            const prt::ChunkPlan p = prt::plan_chunks(num(i), num(i + 1), num(i + 2), (size_t)num(i + 3));
            std::printf("%s[%lld, %lld]", i > 2 ? ", " : "", (long long)p.chunk, (long long)p.n_launches);
        }
        std::printf("]}\n");
    } else if (mode == "frames" && argc == 5) {
        const int64_t spp = num(2), n_frames = num(3), chunk = num(4), T = spp * n_frames;
        std::printf("{\"launches\": [");
        for (int64_t s0 = 0; s0 < T; s0 += chunk) {
            const int64_t n = std::min<int64_t>(chunk, T - s0);
            const prt::FrameSpan f = prt::launch_frames(s0, n, spp, n_frames);
            std::printf("%s[%lld, %lld, %lld, %lld]", s0 ? ", " : "", (long long)s0, (long long)n, (long long)f.f0,
                        (long long)f.f1);
        }
        std::printf("]}\n");
    } else if (mode == "camera" && argc == 3) {
        std::vector<float> cam;
        if (!read_raw(argv[2], &cam) || cam.size() < 21) return 2;
        float o[3], k[3];
        prt::camera_terms(cam.data(), o, k);
        std::printf("{\"fast\": %s, \"cam_o\": [%u, %u, %u], \"cam_k\": [%u, %u, %u]}\n",
                    prt::camera_is_fast(cam.data()) ? "true" : "false", bits(o[0]), bits(o[1]), bits(o[2]), bits(k[0]),
                    bits(k[1]), bits(k[2]));
    } else if (mode == "env" && argc == 6) {
        const long long v = prt::env_int(argv[2], num(3), num(4), num(5));
        std::printf("{\"value\": %lld, \"spill_lds\": %d}\n", v, prt::spill_lds_entries(v));
    } else if (mode == "layout" && argc >= 9 && (argc - 2) % 7 == 0) {
        std::printf("[");
        for (int i = 2; i < argc; i += 7) {
            const prt::LdsSizes z{(int)num(i), (int)num(i + 1), (int)num(i + 2), (int)num(i + 3), (int)num(i + 4),
                                  (int)num(i + 5), (int)num(i + 6)};
            const prt::TraceLds t = prt::trace_lds(z);
            const prt::PoolLds p = prt::pool_lds(z);
            std::printf("%s{\"trace\": ", i > 2 ? ", " : "");
            print_list(std::vector<int64_t>{t.stacks, t.nodes, t.tris, t.normals, t.frames, t.mats, t.light_v,
                                            t.light_off});
            std::printf(", \"trace_bytes\": %zu, \"pool\": ", t.bytes);
            print_list(std::vector<int64_t>{p.stacks, p.pool, p.queue, p.ctl, p.nodes, p.tris, p.light_v, p.light_off,
                                            p.mats});
            std::printf(", \"pool_bytes\": %zu, \"scene_bytes\": %zu, \"smem\": ", p.bytes, prt::lds_scene_bytes(z));
            // trace_smem_bytes of every variant id (and the unknown 0 and 9) at the instantiation set z.stack
            std::vector<size_t> smem;
            for (int var = 0; var <= prt::kVarLast + 1; ++var) smem.push_back(prt::trace_smem_bytes(z.stack, var, z));
            print_list(smem);
            std::printf("}");
        }
        std::printf("]\n");
    } else if (mode == "variant" && argc >= 10 && (argc - 2) % 8 == 0) {
        std::printf("[");
        for (int i = 2; i < argc; i += 8) {
            const int need4 = (int)num(i + 6), stack4 = (int)num(i + 7);
            const prt::LdsSizes z{(int)num(i), (int)num(i + 1), (int)num(i + 2), (int)num(i + 3), (int)num(i + 4),
                                  (int)num(i + 5), need4};
            std::printf("%s{\"fits\": %s, \"nee\": %d, \"mis\": %d}", i > 2 ? ", " : "",
                        prt::lds_fits(z) ? "true" : "false", prt::choose_variant(z, need4, stack4, false),
                        prt::choose_variant(z, need4, stack4, true));
        }
        std::printf("]\n");
    } else if (mode == "width" && argc >= 12 && (argc - 2) % 10 == 0) {
        std::vector<int> w;
        for (int i = 2; i < argc; i += 10) {
            const prt::LdsSizes z8{(int)num(i), (int)num(i + 1), (int)num(i + 2), (int)num(i + 3), (int)num(i + 4),
                                   (int)num(i + 5), (int)num(i + 6), (int)num(i + 7)};
            w.push_back(prt::lds_width(z8, (int)num(i + 8), (int)num(i + 9)));
        }
        std::printf("{\"width\": ");
        print_list(w);
        std::printf("}\n");
    } else if (mode == "scene" && argc == 7) {
        return scene_mode(argv[2], num(3), num(4), (int)num(5), (int)num(6));
    } else {
        std::fprintf(stderr, "usage: see tools/sanitize/host_check.cpp\n");
        return 2;
    }
    return 0;
}

// prt_multi.cpp — prt_render_multi: one frame rendered by several devices, gathered over RCCL.
// librccl is resolved at first use with dlopen (by SONAME first, so a process that already loaded
// torch's RCCL shares that instance and its HIP runtime), which keeps libprt loadable on machines
// without RCCL: only prt_render_multi then fails, with PRT_ERR_RCCL.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <map>
#include <mutex>

#include "prt_host.h"

namespace prt {
namespace {

struct Rccl {
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    ncclResult_t (*send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};

std::mutex g_comm_mu;   // guards g_rccl and g_comms
Rccl g_rccl;
bool g_rccl_tried = false;
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comms;   // per device list (root first)

const Rccl& rccl() {
    if (g_rccl_tried) return g_rccl;
    g_rccl_tried = true;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) {
        g_rccl.why = std::string("librccl.so.1 not loadable: ") + (dlerror() ? dlerror() : "?");
        return g_rccl;
    }
    auto sym = [&](const char* n) { return dlsym(h, n); };
    g_rccl.comm_init_all = (decltype(g_rccl.comm_init_all))sym("ncclCommInitAll");
    g_rccl.comm_destroy = (decltype(g_rccl.comm_destroy))sym("ncclCommDestroy");
    g_rccl.group_start = (decltype(g_rccl.group_start))sym("ncclGroupStart");
    g_rccl.group_end = (decltype(g_rccl.group_end))sym("ncclGroupEnd");
    g_rccl.send = (decltype(g_rccl.send))sym("ncclSend");
    g_rccl.recv = (decltype(g_rccl.recv))sym("ncclRecv");
    g_rccl.error_string = (decltype(g_rccl.error_string))sym("ncclGetErrorString");
    g_rccl.ok = g_rccl.comm_init_all && g_rccl.comm_destroy && g_rccl.group_start && g_rccl.group_end &&
                g_rccl.send && g_rccl.recv && g_rccl.error_string;
    if (!g_rccl.ok) g_rccl.why = "librccl lacks ncclCommInitAll / ncclSend / ncclRecv / group calls";
    return g_rccl;
}

#define RCCL_TRY(expr)                                                                           \
    do {                                                                                         \
        ncclResult_t r_ = (expr);                                                                \
        if (r_ != ncclSuccess) return fail(PRT_ERR_RCCL, std::string(#expr) + ": " + R.error_string(r_)); \
    } while (0)

}  // namespace
}  // namespace prt

using namespace prt;

extern "C" {

int prt_render_multi(void* const* scenes, int n_scenes, const float* cam, int W, int H, int tile, int spp, int depth,
                     uint64_t seed, uint32_t flags, float* out_frame) {
    if (!scenes || n_scenes < 1) return fail(PRT_ERR_ARG, "need at least one scene handle");
    if (!out_frame) return fail(PRT_ERR_ARG, "out_frame is NULL");
    std::vector<Scene*> sc((size_t)n_scenes);
    std::vector<int> devs((size_t)n_scenes);
    for (int r = 0; r < n_scenes; ++r) {
        sc[(size_t)r] = (Scene*)scenes[r];
        if (!sc[(size_t)r]) return fail(PRT_ERR_ARG, "scene handle " + std::to_string(r) + " is NULL");
        devs[(size_t)r] = sc[(size_t)r]->device;
        for (int q = 0; q < r; ++q)
            if (devs[(size_t)q] == devs[(size_t)r])
                return fail(PRT_ERR_ARG, "scene handles must live on distinct devices (device " +
                                             std::to_string(devs[(size_t)r]) + " twice)");
    }
    // tile ownership: the 'latin' interleave of device_scene.tile_owner
    const std::vector<std::vector<int32_t>> ids = latin_tile_ids(W, H, tile, n_scenes);
    for (size_t r = 0; r < ids.size(); ++r)
        if (int rc = check_render_args(sc[r], cam, W, H, tile, tile, ids[r].data(), (int)ids[r].size(), spp, depth))
            return rc;
    std::lock_guard<std::mutex> lock(g_comm_mu);
    const Rccl& R = rccl();
    if (!R.ok) return fail(PRT_ERR_RCCL, R.why);
    auto it = g_comms.find(devs);
    if (it == g_comms.end()) {
        std::vector<ncclComm_t> comms((size_t)n_scenes, nullptr);
        RCCL_TRY(R.comm_init_all(comms.data(), n_scenes, devs.data()));
        it = g_comms.emplace(devs, std::move(comms)).first;
    }
    const std::vector<ncclComm_t>& comms = it->second;
    const int64_t slots = (int64_t)tile * tile;
    const int log_t = __builtin_ctz((unsigned)tile);
    // 1. every rank renders its tiles into its render context's sums (async, own stream)
    std::vector<RenderCtx*> cx((size_t)n_scenes, nullptr);
    std::vector<int64_t> off((size_t)n_scenes + 1, 0);
    for (size_t r = 0; r < ids.size(); ++r) {
        Scene* s = sc[r];
        DeviceGuard g(s->device);
        const int nt = (int)ids[r].size();
        off[r + 1] = off[r] + nt * slots;
        if (int rc = render_ctx(s, s->stream, &cx[r])) return rc;
        HIP_TRY(cx[r]->acc.ensure(std::max<size_t>(16, sizeof(float) * 3 * (size_t)(nt * slots))));
        if (int rc = enqueue_render(s, cx[r], cam, W, H, tile, tile, ids[r].data(), nt, spp, depth, seed, flags,
                                    (float*)cx[r]->acc.p))
            return rc;
    }
    // 2. root buffers: gathered sums of every rank (rank-major) and their tile origins
    Scene* root = sc[0];
    {
        DeviceGuard g(root->device);
        root->gather_xy_host.clear();
        for (const std::vector<int32_t>& t : ids) {
            const std::vector<uint32_t> xy = tile_origins(t.data(), (int64_t)t.size(), (W + tile - 1) / tile, tile, tile);
            root->gather_xy_host.insert(root->gather_xy_host.end(), xy.begin(), xy.end());
        }
        HIP_TRY(root->gather.ensure(sizeof(float) * 3 * (size_t)off[(size_t)n_scenes]));
        HIP_TRY(root->gather_xy.ensure(sizeof(uint32_t) * root->gather_xy_host.size()));
        HIP_TRY(root->frame.ensure(sizeof(float) * 3 * (size_t)W * (size_t)H));
        HIP_TRY(hipMemcpyAsync(root->gather_xy.p, root->gather_xy_host.data(),
                               sizeof(uint32_t) * root->gather_xy_host.size(), hipMemcpyHostToDevice, root->stream));
    }
    // 3. the only exchange: every rank (the root too, through its self-loop) sends its packed
    //    tile sums to the root in one RCCL group (point-to-point over xGMI; RCCL has no gather)
    RCCL_TRY(R.group_start());
    for (int r = 0; r < n_scenes; ++r) {
        const size_t n = (size_t)(off[(size_t)r + 1] - off[(size_t)r]) * 3;
        if (n == 0) continue;
        Scene* s = sc[(size_t)r];
        ncclResult_t e = R.send(cx[(size_t)r]->acc.p, n, ncclFloat32, 0, comms[(size_t)r], s->stream);
        if (e == ncclSuccess)
            e = R.recv((float*)root->gather.p + 3 * off[(size_t)r], n, ncclFloat32, r, comms[0], root->stream);
        if (e != ncclSuccess) {
            (void)R.group_end();
            return fail(PRT_ERR_RCCL, std::string("ncclSend/ncclRecv: ") + R.error_string(e));
        }
    }
    RCCL_TRY(R.group_end());
    // 4. root: tiles -> [x][y] frame, frame -> host
    {
        DeviceGuard g(root->device);
        HIP_TRY(launch_scatter((const float*)root->gather.p, (const uint32_t*)root->gather_xy.p,
                               (int)off[(size_t)n_scenes], log_t, 2 * log_t, 0, 0, W, H, (float*)root->frame.p,
                               root->stream));
        HIP_TRY(hipMemcpyAsync(out_frame, root->frame.p, sizeof(float) * 3 * (size_t)W * (size_t)H,
                               hipMemcpyDeviceToHost, root->stream));
    }
    for (int r = 0; r < n_scenes; ++r) {
        DeviceGuard g(sc[(size_t)r]->device);
        HIP_TRY(hipStreamSynchronize(sc[(size_t)r]->stream));
        if (take_fault_at(cx[(size_t)r]->work) != 0)
            return fail(PRT_ERR_INTERNAL, "traversal watchdog tripped on device " + std::to_string(devs[(size_t)r]));
    }
    return PRT_OK;
}

void prt_comm_release(void) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    if (g_rccl.ok)
        for (auto& kv : g_comms)
            for (ncclComm_t c : kv.second) (void)g_rccl.comm_destroy(c);
    g_comms.clear();
}

}  // extern "C"

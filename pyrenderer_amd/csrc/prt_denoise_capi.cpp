// prt_denoise_capi.cpp — the extern "C" surface of the a-trous denoiser (include/prt.h, "denoise").
//
// A unit of its own next to prt_capi.cpp: it keeps its own thread-local error text
// (prt_denoise_last_error) and shares no state with the scene code.  Arguments are checked
// before any HIP call, so a rejected call never touches a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prt.h"
#include "prt_denoise.h"

namespace {

thread_local std::string g_dn_err;

int fail(int code, const std::string& msg) {
    g_dn_err = msg;
    return code;
}

#define DN_HIP_TRY(expr)                                                                                       \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return fail(PRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

#define DN_TRY(expr)                  \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_ != PRT_OK) return rc_; \
    } while (0)

// The last step before an entry point enqueues anything, and the first that touches HIP: enter() checks the
// device ordinal against the visible devices (PRT_ERR_HIP without a device, PRT_ERR_ARG out of range; an
// invalid ordinal must not run on whatever device was current) and makes it current for the guard's lifetime.
struct DeviceGuard {
    int prev = -1;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }

    int enter(const std::string& who, int device) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
            (void)hipGetLastError();
            return fail(PRT_ERR_HIP, who + ": no HIP device");
        }
        if (device >= n_dev) return fail(PRT_ERR_ARG, who + ": no such device");
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        const hipError_t err = hipSetDevice(device);   // its failure keeps the text it has always had
        if (err != hipSuccess) return fail(PRT_ERR_HIP, std::string("g.err: ") + hipGetErrorString(err));
        return PRT_OK;
    }
};

// Device buffers of a host-form entry point, freed when it returns.  The buffers are allocated first,
// one after the other (after a failure nothing more is allocated and oom() tells); then upload() copies
// in every buffer that has a source and, after the kernels, download() copies out every one that has
// a destination.  The copies on the null stream follow the kernels and block until they are done.
class Staging {
    struct Buf {
        void* d;
        const void* from;
        void* to;
        size_t bytes;
    };
    std::vector<Buf> bufs_;
    bool oom_ = false;

    hipError_t copy(bool up) const {
        for (const Buf& b : bufs_) {
            hipError_t e = hipSuccess;
            if (up && b.from) e = hipMemcpy(b.d, b.from, b.bytes, hipMemcpyHostToDevice);
            if (!up && b.to) e = hipMemcpy(b.to, b.d, b.bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }

public:
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() { for (const Buf& b : bufs_) (void)hipFree(b.d); }

    void* bytes(size_t n_bytes, const void* from = nullptr, void* to = nullptr) {
        void* d = nullptr;
        if (oom_ || hipMalloc(&d, n_bytes) != hipSuccess) {
            oom_ = true;
            return nullptr;
        }
        bufs_.push_back({d, from, to, n_bytes});
        return d;
    }
    // an input of no floats (an empty motion table, whose `host` may be null) and an output nobody asked for
    // (a null `host`): nothing is allocated
    const float* in(const float* host, size_t count) {
        return count ? static_cast<float*>(bytes(count * sizeof(float), host)) : nullptr;
    }
    float* out(float* host, size_t count) {
        return host ? static_cast<float*>(bytes(count * sizeof(float), nullptr, host)) : nullptr;
    }
    float* inout(float* host, size_t count) { return static_cast<float*>(bytes(count * sizeof(float), host, host)); }
    bool oom() const { return oom_; }
    hipError_t upload() const { return copy(true); }
    hipError_t download() const { return copy(false); }
};

int fail_oom(const std::string& who) {
    (void)hipGetLastError();
    return fail(PRT_ERR_OOM, who + ": device allocation failed");
}

bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

// what is wrong with a frame's shape; empty when nothing is
std::string frame_fault(int W, int H) {
    if (W < 1 || H < 1) return "W and H must be >= 1";
    if (W > prt_dn::kMaxSide || H > prt_dn::kMaxSide) return "W and H must be <= " + std::to_string(prt_dn::kMaxSide);
    return "";
}

// device ordinal and frame shape, shared by every entry point
int check_frame(const std::string& who, int device, int W, int H) {
    if (device < 0) return fail(PRT_ERR_ARG, who + ": device < 0");
    const std::string fault = frame_fault(W, H);
    if (!fault.empty()) return fail(PRT_ERR_ARG, who + ": " + fault);
    return PRT_OK;
}

// the two *_work_bytes exports: 0 for a frame that check_frame refuses, and no error text
int64_t work_bytes_or_0(int W, int H, bool variance) {
    return frame_fault(W, H).empty() ? (int64_t)prt_dn::work_bytes(W, H, variance) : 0;
}

int check_iterations(const std::string& who, int iterations) {
    if (iterations < 0 || iterations > prt_dn::kMaxIterations)
        return fail(PRT_ERR_ARG, who + ": iterations must be in 0.." + std::to_string(prt_dn::kMaxIterations));
    return PRT_OK;
}

// shape and parameter checks of the fixed filter's entry points; fills `p`
int check_args(const std::string& who, int device, int W, int H, int iterations, const float* params4,
               prt_dn::FilterParams* p) {
    DN_TRY(check_frame(who, device, W, H));
    DN_TRY(check_iterations(who, iterations));
    if (!params4) return fail(PRT_ERR_ARG, who + ": params4 is NULL");
    *p = {params4[0], params4[1], params4[2], params4[3], 0.0f};   // sigma = sigma_c; no eps_l
    if (!positive_finite(p->sigma) || !positive_finite(p->sigma_z))
        return fail(PRT_ERR_ARG, who + ": sigma_c and sigma_z must be positive and finite");
    if (!positive_finite(p->eps_a) || !positive_finite(p->eps_z))
        return fail(PRT_ERR_ARG, who + ": eps_a and eps_z must be positive and finite");
    // the last pass divides by (sigma_c * 2^-i)^2: it must not underflow to 0 or overflow
    const float sc_last = p->sigma * (1.0f / (float)(1 << (iterations > 0 ? iterations - 1 : 0)));
    if (!positive_finite(sc_last * sc_last) || !positive_finite(p->sigma * p->sigma))
        return fail(PRT_ERR_ARG, who + ": sigma_c squared leaves the f32 range");
    return PRT_OK;
}

// check_args for the variance-guided entry points (params5 = sigma_l, sigma_z, eps_a, eps_z, eps_l)
int check_var_args(const std::string& who, int device, int W, int H, int iterations, const float* params5,
                   prt_dn::FilterParams* p) {
    DN_TRY(check_frame(who, device, W, H));
    DN_TRY(check_iterations(who, iterations));
    if (!params5) return fail(PRT_ERR_ARG, who + ": params5 is NULL");
    *p = {params5[0], params5[1], params5[2], params5[3], params5[4]};   // sigma = sigma_l
    if (!positive_finite(p->sigma) || !positive_finite(p->sigma_z))
        return fail(PRT_ERR_ARG, who + ": sigma_l and sigma_z must be positive and finite");
    if (!positive_finite(p->eps_a) || !positive_finite(p->eps_z) || !positive_finite(p->eps_l))
        return fail(PRT_ERR_ARG, who + ": eps_a, eps_z and eps_l must be positive and finite");
    return PRT_OK;
}

// checks of the moments entry points; a frame_pitch of 0 (packed) is replaced by W * H * 3
int check_moments_args(const std::string& who, int device, int n_frames, int64_t* frame_pitch, float n_samples,
                       float eps_a, int W, int H) {
    DN_TRY(check_frame(who, device, W, H));
    if (n_frames < 1) return fail(PRT_ERR_ARG, who + ": n_frames must be >= 1");
    const int64_t packed = (int64_t)W * (int64_t)H * 3;
    if (*frame_pitch == 0) *frame_pitch = packed;
    if (*frame_pitch < packed) return fail(PRT_ERR_ARG, who + ": frame_pitch must be 0 or >= W * H * 3");
    if (*frame_pitch > INT64_MAX / 4 / (int64_t)n_frames)
        return fail(PRT_ERR_ARG, who + ": n_frames * frame_pitch leaves the address range");
    if (!std::isfinite(n_samples) || n_samples < 1.0f)
        return fail(PRT_ERR_ARG, who + ": n_samples must be finite and >= 1");
    if (!positive_finite(eps_a)) return fail(PRT_ERR_ARG, who + ": eps_a must be positive and finite");
    return PRT_OK;
}

// Checks of the adaptive entry points that come before the tile list is read: the frame, the tile shape (the
// render calls' rule), the samples per batch and params2 = eps_r, target; fills `p`.
int check_adaptive_params(const std::string& who, int device, int n_tiles, int tw, int th, int W, int H, float eps_a,
                          float n_samples, const float* params2, prt_dn::AdaptiveParams* p) {
    DN_TRY(check_frame(who, device, W, H));
    if (tw < 1 || th < 1 || (tw & (tw - 1)) || (th & (th - 1)) || (int64_t)tw * th < prt_dn::kMinTilePixels ||
        (int64_t)tw * th > prt_dn::kMaxTilePixels)
        return fail(PRT_ERR_ARG, who + ": tw and th must be powers of two with tw * th in 64..2^20");
    if (n_tiles < 0) return fail(PRT_ERR_ARG, who + ": n_tiles must be >= 0");
    if ((int64_t)n_tiles * tw * th >= ((int64_t)1 << 31))
        return fail(PRT_ERR_ARG, who + ": n_tiles * tw * th must stay below 2^31 slots");
    if (!std::isfinite(n_samples) || n_samples < 1.0f)
        return fail(PRT_ERR_ARG, who + ": n_samples must be finite and >= 1");
    if (!positive_finite(eps_a)) return fail(PRT_ERR_ARG, who + ": eps_a must be positive and finite");
    if (!params2) return fail(PRT_ERR_ARG, who + ": params2 is NULL");
    *p = {n_samples, eps_a, params2[0], params2[1]};
    if (!positive_finite(p->eps_r)) return fail(PRT_ERR_ARG, who + ": eps_r must be positive and finite");
    if (!(p->target >= 0.0f)) return fail(PRT_ERR_ARG, who + ": target must be >= 0 (+inf is allowed), not NaN");
    return PRT_OK;
}

// The tile list of an adaptive call: every id inside the frame's tile grid and none listed twice.  No index is
// formed from an id before this has passed.
int check_tile_list(const std::string& who, const int32_t* tile_ids, int n_tiles, int tw, int th, int W, int H) {
    const int64_t n_grid = (int64_t)((W + tw - 1) / tw) * (int64_t)((H + th - 1) / th);
    for (int i = 0; i < n_tiles; ++i)
        if (tile_ids[i] < 0 || tile_ids[i] >= n_grid)
            return fail(PRT_ERR_ARG, who + ": tile id out of range: " + std::to_string(tile_ids[i]));
    std::vector<int32_t> sorted(tile_ids, tile_ids + n_tiles);
    std::sort(sorted.begin(), sorted.end());
    const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
    if (twice != sorted.end())
        return fail(PRT_ERR_ARG, who + ": tile id listed twice: " + std::to_string(*twice) +
                                       " (two blocks would update the same pixels)");
    return PRT_OK;
}

// a caller's scratch (not NULL: the entry point has looked) against `need`, the value of `need_fn`(W, H)
int check_scratch(const std::string& who, const void* d_work, int64_t work_bytes, size_t need, const char* need_fn) {
    if (work_bytes < (int64_t)need)
        return fail(PRT_ERR_ARG, who + ": d_work is smaller than " + need_fn + "(W, H)");
    if (reinterpret_cast<uintptr_t>(d_work) % 16 != 0) return fail(PRT_ERR_ARG, who + ": d_work must be 16-byte aligned");
    return PRT_OK;
}

// aliasing rules of the device entry points; d_out_var and d_in_var may be null
int check_aliasing(const std::string& who, const float* d_color, const float* d_feat, const float* d_out,
                   const float* d_out_var, const float* d_in_var) {
    if (d_out == d_color) return fail(PRT_ERR_ARG, who + ": d_out must not alias d_color");
    if (d_out_var && (d_out_var == d_out || d_out_var == d_color || d_out_var == d_feat))
        return fail(PRT_ERR_ARG, who + ": d_out_var must not alias d_out, d_color or d_feat");
    if (d_in_var && (d_in_var == d_out || d_in_var == d_out_var))
        return fail(PRT_ERR_ARG, who + ": d_in_var must not alias d_out or d_out_var");
    return PRT_OK;
}

using prt_dn::Mode;

// what a mode's entry points differ in: the fixed filter has no variance planes, and only a given or a
// mixed variance needs the caller's plane
bool has_variance(Mode m) { return m != Mode::kFixed; }
bool needs_plane(Mode m) { return m == Mode::kGiven || m == Mode::kMixed; }

int check_filter_args(const std::string& who, Mode mode, int device, int W, int H, int iterations, const float* params,
                      prt_dn::FilterParams* p) {
    return has_variance(mode) ? check_var_args(who, device, W, H, iterations, params, p)
                              : check_args(who, device, W, H, iterations, params, p);
}

// the device form of all four filters: prt_denoise_device, prt_denoise_var_device, prt_denoise_var_given_device
// and prt_denoise_var_mixed_device.  d_in_var is null where the mode needs no plane, d_out_var for the fixed filter.
int filter_device(const std::string& who, Mode mode, int device, const float* d_color, const float* d_feat,
                  const float* d_in_var, int W, int H, int iterations, const float* params, float* d_out,
                  float* d_out_var, void* d_work, int64_t work_bytes, void* stream) {
    prt_dn::FilterParams p;
    if (!d_color || !d_feat || (needs_plane(mode) && !d_in_var) || !d_out || !d_work) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_filter_args(who, mode, device, W, H, iterations, params, &p));
    DN_TRY(check_scratch(who, d_work, work_bytes, prt_dn::work_bytes(W, H, has_variance(mode)),
                         has_variance(mode) ? "prt_denoise_var_work_bytes" : "prt_denoise_work_bytes"));
    DN_TRY(check_aliasing(who, d_color, d_feat, d_out, d_out_var, d_in_var));
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    DN_HIP_TRY(prt_dn::enqueue_filter(mode, d_color, d_feat, d_in_var, W, H, iterations, p, d_out, d_out_var, d_work,
                                      static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

// the host form of all four: prt_denoise, prt_denoise_var, prt_denoise_var_given and prt_denoise_var_mixed
int filter_host(const std::string& who, Mode mode, int device, const float* color, const float* feat, const float* in_var,
                int W, int H, int iterations, const float* params, float* out, float* out_var) {
    prt_dn::FilterParams p;
    if (!color || !feat || (needs_plane(mode) && !in_var) || !out) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_filter_args(who, mode, device, W, H, iterations, params, &p));
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    const size_t n = (size_t)W * (size_t)H;
    Staging s;
    const float* d_color = s.in(color, n * 3);
    const float* d_feat = s.in(feat, n * 8);
    const float* d_in_var = needs_plane(mode) ? s.in(in_var, n) : nullptr;
    float* d_out = s.out(out, n * 3);
    float* d_out_var = s.out(out_var, n);
    void* d_work = s.bytes(prt_dn::work_bytes(W, H, has_variance(mode)));
    if (s.oom()) return fail_oom(who);
    DN_HIP_TRY(s.upload());
    DN_HIP_TRY(prt_dn::enqueue_filter(mode, d_color, d_feat, d_in_var, W, H, iterations, p, d_out, d_out_var, d_work, nullptr));
    DN_HIP_TRY(s.download());
    return PRT_OK;
}

// checks of the temporal entry points that need no pointer: the frame and params8 = alpha, alpha_m, tau_n,
// tau_z, tau_a, eps_a, min_history, w_min; fills `p`.  A comparison with a NaN is false, so each range is
// written as the condition a legal value meets.
int check_temporal_params(const std::string& who, int device, int W, int H, const float* params8,
                          prt_dn::TemporalParams* p) {
    DN_TRY(check_frame(who, device, W, H));
    if (!params8) return fail(PRT_ERR_ARG, who + ": params8 is NULL");
    *p = {params8[0], params8[1], params8[2], params8[3], params8[4], params8[5], params8[6], params8[7]};
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f)) return fail(PRT_ERR_ARG, who + ": alpha must be in [0, 1]");
    if (!(p->alpha_m >= 0.0f && p->alpha_m <= 1.0f)) return fail(PRT_ERR_ARG, who + ": alpha_m must be in [0, 1]");
    if (!(p->tau_n >= -1.0f && p->tau_n <= 1.0f)) return fail(PRT_ERR_ARG, who + ": tau_n must be in [-1, 1]");
    if (!positive_finite(p->tau_z)) return fail(PRT_ERR_ARG, who + ": tau_z must be positive and finite");
    if (!(p->tau_a >= 0.0f && std::isfinite(p->tau_a))) return fail(PRT_ERR_ARG, who + ": tau_a must be >= 0 and finite");
    if (!positive_finite(p->eps_a)) return fail(PRT_ERR_ARG, who + ": eps_a must be positive and finite");
    if (!(p->min_history >= 1.0f && std::isfinite(p->min_history)))
        return fail(PRT_ERR_ARG, who + ": min_history must be >= 1 and finite");
    if (!(p->w_min > 0.0f && p->w_min <= 1.0f)) return fail(PRT_ERR_ARG, who + ": w_min must be in (0, 1]");
    return PRT_OK;
}

// the camera records of a temporal call: the three `prev` pointers are NULL together (the first frame) or
// not at all, every float is finite, and neither camera has an aperture (a thin lens has no unique
// reprojection).  `is_static`: the two records are bytewise equal.
int check_temporal_cameras(const std::string& who, const float* cam24, const void* prev_feat, const float* prev_cam24,
                           const void* prev_state, bool* is_static) {
    const int n_prev = (prev_feat ? 1 : 0) + (prev_cam24 ? 1 : 0) + (prev_state ? 1 : 0);
    if (n_prev != 0 && n_prev != 3)
        return fail(PRT_ERR_ARG, who + ": prev_feat, prev_cam24 and prev_state must be NULL together or not at all");
    for (const float* cam : {cam24, prev_cam24}) {
        if (!cam) continue;
        for (int i = 0; i < PRT_CAM_FLOATS; ++i)
            if (!std::isfinite(cam[i])) return fail(PRT_ERR_ARG, who + ": a camera record is not finite");
        if (cam[19] > 0.0f) return fail(PRT_ERR_ARG, who + ": a camera with an aperture > 0 cannot be reprojected");
    }
    *is_static = prev_cam24 && std::memcmp(cam24, prev_cam24, PRT_CAM_FLOATS * sizeof(float)) == 0;
    return PRT_OK;
}

// NULL pointers, parameters, cameras and, with motion, the id planes and the table: everything the two forms of
// a temporal entry point check alike
int check_temporal_args(const std::string& who, const prt_dn::Motion* m, int device, const float* color, const float* feat,
                        const float* cam24, const float* prev_feat, const float* prev_cam24, const float* prev_state,
                        int W, int H, const float* params8, const float* state, prt_dn::TemporalParams* p,
                        bool* is_static) {
    if (!color || !feat || !cam24 || !state || (m && !m->ids)) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_temporal_params(who, device, W, H, params8, p));
    DN_TRY(check_temporal_cameras(who, cam24, prev_feat, prev_cam24, prev_state, is_static));
    if (!m) return PRT_OK;
    if ((m->prev_ids != nullptr) != (prev_state != nullptr))
        return fail(PRT_ERR_ARG, who + ": prev_ids must be NULL together with prev_feat, prev_cam24 and prev_state or not at all");
    if (m->n_objects < 0 || m->n_objects > prt_dn::kMaxObjects)
        return fail(PRT_ERR_ARG, who + ": n_objects must be in 0.." + std::to_string(prt_dn::kMaxObjects));
    if (m->n_objects > 0 && !m->rows) return fail(PRT_ERR_ARG, who + ": motion is NULL with n_objects > 0");
    return PRT_OK;
}

// the device form of both temporal entry points; `m` holds device pointers
int temporal_device(const std::string& who, const prt_dn::Motion* m, int device, const float* d_color, const float* d_feat,
                    const float* cam24, const float* d_prev_feat, const float* prev_cam24, const float* d_prev_state,
                    int W, int H, const float* params8, float* d_state, float* d_out_color, float* d_out_var,
                    void* stream) {
    prt_dn::TemporalParams p;
    bool is_static = false;
    DN_TRY(check_temporal_args(who, m, device, d_color, d_feat, cam24, d_prev_feat, prev_cam24, d_prev_state, W, H,
                               params8, d_state, &p, &is_static));
    if (reinterpret_cast<uintptr_t>(d_state) % 16 != 0 || reinterpret_cast<uintptr_t>(d_prev_state) % 16 != 0)
        return fail(PRT_ERR_ARG, who + ": d_state and d_prev_state must be 16-byte aligned");
    if (m && (reinterpret_cast<uintptr_t>(m->ids) % 4 != 0 || reinterpret_cast<uintptr_t>(m->prev_ids) % 4 != 0 ||
              reinterpret_cast<uintptr_t>(m->rows) % 4 != 0))
        return fail(PRT_ERR_ARG, who + ": d_ids, d_prev_ids and d_motion must be 4-byte aligned");
    // every output against every input and against the other outputs
    const void* ins[] = {d_color, d_feat, d_prev_feat, d_prev_state, m ? m->ids : nullptr, m ? m->prev_ids : nullptr,
                         m ? m->rows : nullptr};
    const void* outs[] = {d_state, d_out_color, d_out_var};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        for (const void* in : ins)
            if (outs[i] == in)
                return fail(PRT_ERR_ARG, who + ": d_state, d_out_color and d_out_var must not alias an input (d_state "
                                               "not d_prev_state: taps read neighbours)");
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return fail(PRT_ERR_ARG, who + ": d_state, d_out_color and d_out_var must not alias each other");
    }
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    DN_HIP_TRY(prt_dn::enqueue_temporal(d_color, d_feat, cam24, d_prev_feat, prev_cam24, d_prev_state, m, W, H, is_static,
                                        p, d_state, d_out_color, d_out_var, static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

// the host form of both; `m` holds host pointers, its planes and table are staged like the rest
int temporal_host(const std::string& who, const prt_dn::Motion* m, int device, const float* color, const float* feat,
                  const float* cam24, const float* prev_feat, const float* prev_cam24, const float* prev_state, int W,
                  int H, const float* params8, float* state, float* out_color, float* out_var) {
    prt_dn::TemporalParams p;
    bool is_static = false;
    DN_TRY(check_temporal_args(who, m, device, color, feat, cam24, prev_feat, prev_cam24, prev_state, W, H, params8, state,
                               &p, &is_static));
    if (state == prev_state) return fail(PRT_ERR_ARG, who + ": state must not alias prev_state");
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    const size_t n = (size_t)W * (size_t)H;
    Staging s;
    const float* d_color = s.in(color, n * 3);
    const float* d_feat = s.in(feat, n * 8);
    const float* d_prev_feat = prev_feat ? s.in(prev_feat, n * 8) : nullptr;
    const float* d_prev_state = prev_state ? s.in(prev_state, n * prt_dn::kTemporalChannels) : nullptr;
    prt_dn::Motion d_m = {nullptr, nullptr, nullptr, 0};
    if (m) {
        d_m.ids = static_cast<const int32_t*>(s.bytes(n * sizeof(int32_t), m->ids));
        if (m->prev_ids) d_m.prev_ids = static_cast<const int32_t*>(s.bytes(n * sizeof(int32_t), m->prev_ids));
        d_m.rows = s.in(m->rows, (size_t)m->n_objects * 12);
        d_m.n_objects = m->n_objects;
    }
    float* d_state = s.out(state, n * prt_dn::kTemporalChannels);
    float* d_out_color = s.out(out_color, n * 3);
    float* d_out_var = s.out(out_var, n);
    if (s.oom()) return fail_oom(who);
    DN_HIP_TRY(s.upload());
    DN_HIP_TRY(prt_dn::enqueue_temporal(d_color, d_feat, cam24, d_prev_feat, prev_cam24, d_prev_state, m ? &d_m : nullptr,
                                        W, H, is_static, p, d_state, d_out_color, d_out_var, nullptr));
    DN_HIP_TRY(s.download());
    return PRT_OK;
}

}  // namespace

extern "C" {

const char* prt_denoise_last_error(void) { return g_dn_err.c_str(); }

int64_t prt_denoise_work_bytes(int W, int H) { return work_bytes_or_0(W, H, false); }

int prt_denoise_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                       const float* params4, float* d_out, void* d_work, int64_t work_bytes, void* stream) {
    return filter_device("prt_denoise_device", Mode::kFixed, device, d_color, d_feat, nullptr, W, H, iterations, params4,
                         d_out, nullptr, d_work, work_bytes, stream);
}

int prt_denoise(int device, const float* color, const float* feat, int W, int H, int iterations,
                const float* params4, float* out) {
    return filter_host("prt_denoise", Mode::kFixed, device, color, feat, nullptr, W, H, iterations, params4, out, nullptr);
}

int64_t prt_denoise_var_work_bytes(int W, int H) { return work_bytes_or_0(W, H, true); }

int prt_denoise_var_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                           const float* params5, float* d_out, float* d_out_var, void* d_work, int64_t work_bytes,
                           void* stream) {
    return filter_device("prt_denoise_var_device", Mode::kEstimate, device, d_color, d_feat, nullptr, W, H, iterations,
                         params5, d_out, d_out_var, d_work, work_bytes, stream);
}

int prt_denoise_var(int device, const float* color, const float* feat, int W, int H, int iterations,
                    const float* params5, float* out, float* out_var) {
    return filter_host("prt_denoise_var", Mode::kEstimate, device, color, feat, nullptr, W, H, iterations, params5, out,
                       out_var);
}

// ---- variance from per-pixel sample moments ----

int prt_denoise_var_given_device(int device, const float* d_color, const float* d_feat, const float* d_in_var,
                                 int W, int H, int iterations, const float* params5, float* d_out,
                                 float* d_out_var, void* d_work, int64_t work_bytes, void* stream) {
    return filter_device("prt_denoise_var_given_device", Mode::kGiven, device, d_color, d_feat, d_in_var, W, H, iterations,
                         params5, d_out, d_out_var, d_work, work_bytes, stream);
}

int prt_denoise_var_given(int device, const float* color, const float* feat, const float* in_var, int W, int H,
                          int iterations, const float* params5, float* out, float* out_var) {
    return filter_host("prt_denoise_var_given", Mode::kGiven, device, color, feat, in_var, W, H, iterations, params5, out,
                       out_var);
}

int prt_moments_add_device(int device, const float* d_sums, int n_frames, int64_t frame_pitch, float n_samples,
                           const float* d_feat, float eps_a, int W, int H, float* d_io_state, void* stream) {
    const std::string who("prt_moments_add_device");
    if (!d_sums || !d_feat || !d_io_state) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_moments_args(who, device, n_frames, &frame_pitch, n_samples, eps_a, W, H));
    if (reinterpret_cast<uintptr_t>(d_io_state) % 16 != 0)
        return fail(PRT_ERR_ARG, who + ": d_io_state must be 16-byte aligned");
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    DN_HIP_TRY(prt_dn::enqueue_moments(d_sums, n_frames, (size_t)frame_pitch, n_samples, d_feat, eps_a, W, H, d_io_state,
                                       static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_moments_add(int device, const float* sums, int n_frames, int64_t frame_pitch, float n_samples,
                    const float* feat, float eps_a, int W, int H, float* io_state) {
    const std::string who("prt_moments_add");
    if (!sums || !feat || !io_state) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_moments_args(who, device, n_frames, &frame_pitch, n_samples, eps_a, W, H));
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    const size_t n = (size_t)W * (size_t)H;
    Staging s;
    // the frames as they lie in the caller's memory, gaps of a pitch included
    const float* d_sums = s.in(sums, (size_t)(n_frames - 1) * (size_t)frame_pitch + n * 3);
    const float* d_feat = s.in(feat, n * 8);
    float* d_state = s.inout(io_state, n * 4);
    if (s.oom()) return fail_oom(who);
    DN_HIP_TRY(s.upload());
    DN_HIP_TRY(prt_dn::enqueue_moments(d_sums, n_frames, (size_t)frame_pitch, n_samples, d_feat, eps_a, W, H, d_state,
                                       nullptr));
    DN_HIP_TRY(s.download());
    return PRT_OK;
}

// ---- variance plane with a spatial fallback ----

int prt_denoise_var_mixed_device(int device, const float* d_color, const float* d_feat, const float* d_in_var,
                                 int W, int H, int iterations, const float* params5, float* d_out,
                                 float* d_out_var, void* d_work, int64_t work_bytes, void* stream) {
    return filter_device("prt_denoise_var_mixed_device", Mode::kMixed, device, d_color, d_feat, d_in_var, W, H, iterations,
                      params5, d_out, d_out_var, d_work, work_bytes, stream);
}

int prt_denoise_var_mixed(int device, const float* color, const float* feat, const float* in_var, int W, int H,
                          int iterations, const float* params5, float* out, float* out_var) {
    return filter_host("prt_denoise_var_mixed", Mode::kMixed, device, color, feat, in_var, W, H, iterations, params5, out,
                    out_var);
}

// ---- temporal accumulation ----

int prt_temporal_accumulate_device(int device, const float* d_color, const float* d_feat, const float* cam24,
                                   const float* d_prev_feat, const float* prev_cam24, const float* d_prev_state,
                                   int W, int H, const float* params8, float* d_state, float* d_out_color,
                                   float* d_out_var, void* stream) {
    return temporal_device("prt_temporal_accumulate_device", nullptr, device, d_color, d_feat, cam24, d_prev_feat,
                           prev_cam24, d_prev_state, W, H, params8, d_state, d_out_color, d_out_var, stream);
}

int prt_temporal_accumulate(int device, const float* color, const float* feat, const float* cam24,
                            const float* prev_feat, const float* prev_cam24, const float* prev_state, int W, int H,
                            const float* params8, float* state, float* out_color, float* out_var) {
    return temporal_host("prt_temporal_accumulate", nullptr, device, color, feat, cam24, prev_feat, prev_cam24,
                         prev_state, W, H, params8, state, out_color, out_var);
}

int prt_temporal_accumulate_motion_device(int device, const float* d_color, const float* d_feat, const float* cam24,
                                          const float* d_prev_feat, const float* prev_cam24,
                                          const float* d_prev_state, const int32_t* d_ids, const int32_t* d_prev_ids,
                                          const float* d_motion, int n_objects, int W, int H, const float* params8,
                                          float* d_state, float* d_out_color, float* d_out_var, void* stream) {
    const prt_dn::Motion m = {d_ids, d_prev_ids, d_motion, n_objects};
    return temporal_device("prt_temporal_accumulate_motion_device", &m, device, d_color, d_feat, cam24, d_prev_feat,
                           prev_cam24, d_prev_state, W, H, params8, d_state, d_out_color, d_out_var, stream);
}

int prt_temporal_accumulate_motion(int device, const float* color, const float* feat, const float* cam24,
                                   const float* prev_feat, const float* prev_cam24, const float* prev_state,
                                   const int32_t* ids, const int32_t* prev_ids, const float* motion, int n_objects,
                                   int W, int H, const float* params8, float* state, float* out_color, float* out_var) {
    const prt_dn::Motion m = {ids, prev_ids, motion, n_objects};
    return temporal_host("prt_temporal_accumulate_motion", &m, device, color, feat, cam24, prev_feat, prev_cam24,
                         prev_state, W, H, params8, state, out_color, out_var);
}

// ---- adaptive sampling ----

int prt_adaptive_update_device(int device, const float* d_batch, const int32_t* tile_ids, int n_tiles, int tw, int th,
                               int W, int H, const float* d_feat, float eps_a, float n_samples, const float* params2,
                               float* d_io_sum, float* d_io_state, uint32_t* d_records, void* stream) {
    const std::string who("prt_adaptive_update_device");
    prt_dn::AdaptiveParams p;
    DN_TRY(check_adaptive_params(who, device, n_tiles, tw, th, W, H, eps_a, n_samples, params2, &p));
    if (n_tiles == 0) return PRT_OK;
    if (!d_batch || !tile_ids || !d_feat || !d_io_sum || !d_io_state || !d_records)
        return fail(PRT_ERR_ARG, who + ": NULL pointer");
    if (reinterpret_cast<uintptr_t>(d_io_state) % 16 != 0)
        return fail(PRT_ERR_ARG, who + ": d_io_state must be 16-byte aligned");
    DN_TRY(check_tile_list(who, tile_ids, n_tiles, tw, th, W, H));
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    DN_HIP_TRY(prt_dn::enqueue_adaptive(d_batch, tile_ids, n_tiles, tw, th, W, H, d_feat, p, d_io_sum, d_io_state,
                                        d_records, static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_adaptive_update(int device, const float* batch, const int32_t* tile_ids, int n_tiles, int tw, int th, int W,
                        int H, const float* feat, float eps_a, float n_samples, const float* params2, float* io_sum,
                        float* io_state, uint32_t* records) {
    const std::string who("prt_adaptive_update");
    prt_dn::AdaptiveParams p;
    DN_TRY(check_adaptive_params(who, device, n_tiles, tw, th, W, H, eps_a, n_samples, params2, &p));
    if (n_tiles == 0) return PRT_OK;
    if (!batch || !tile_ids || !feat || !io_sum || !io_state || !records) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    DN_TRY(check_tile_list(who, tile_ids, n_tiles, tw, th, W, H));
    DeviceGuard g;
    DN_TRY(g.enter(who, device));
    const size_t n = (size_t)W * (size_t)H;
    Staging s;
    // the planes travel whole: the pixels of tiles not listed come back with the bits they went up with
    const float* d_batch = s.in(batch, (size_t)n_tiles * (size_t)tw * (size_t)th * 3);
    const float* d_feat = s.in(feat, n * 8);
    float* d_sum = s.inout(io_sum, n * 3);
    float* d_state = s.inout(io_state, n * 4);
    uint32_t* d_records = static_cast<uint32_t*>(s.bytes((size_t)n_tiles * 4 * sizeof(uint32_t), nullptr, records));
    if (s.oom()) return fail_oom(who);
    DN_HIP_TRY(s.upload());
    DN_HIP_TRY(prt_dn::enqueue_adaptive(d_batch, tile_ids, n_tiles, tw, th, W, H, d_feat, p, d_sum, d_state, d_records,
                                        nullptr));
    DN_HIP_TRY(s.download());
    return PRT_OK;
}

}  // extern "C"

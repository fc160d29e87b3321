// prt_denoise_capi.cpp — the extern "C" surface of the a-trous denoiser (include/prt.h, "denoise").
//
// A unit of its own next to prt_capi.cpp: it keeps its own thread-local error text
// (prt_denoise_last_error) and shares no state with the scene code.  Arguments are checked
// before any HIP call, so a rejected call never touches a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

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

// Makes `dev` current for its lifetime; `err` is hipSetDevice's result, which the caller checks
// before it enqueues anything (an invalid ordinal must not run on whatever device was current).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = hipSetDevice(dev);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// device ordinal against the visible devices: PRT_ERR_HIP without a device, PRT_ERR_ARG out of range
int check_device(const char* fn, int device) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) {
        (void)hipGetLastError();
        return fail(PRT_ERR_HIP, std::string(fn) + ": no HIP device");
    }
    if (device >= n_dev) return fail(PRT_ERR_ARG, std::string(fn) + ": no such device");
    return PRT_OK;
}

struct DevMem {
    void* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { if (p) (void)hipFree(p); }
};

bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

// shape and parameter checks shared by both entry points; fills `p`
int check_args(const char* fn, int device, int W, int H, int iterations, const float* params4, prt_dn::Params* p) {
    const std::string who(fn);
    if (device < 0) return fail(PRT_ERR_ARG, who + ": device < 0");
    if (W < 1 || H < 1) return fail(PRT_ERR_ARG, who + ": W and H must be >= 1");
    if (W > prt_dn::kMaxSide || H > prt_dn::kMaxSide)
        return fail(PRT_ERR_ARG, who + ": W and H must be <= " + std::to_string(prt_dn::kMaxSide));
    if (iterations < 0 || iterations > prt_dn::kMaxIterations)
        return fail(PRT_ERR_ARG, who + ": iterations must be in 0.." + std::to_string(prt_dn::kMaxIterations));
    if (!params4) return fail(PRT_ERR_ARG, who + ": params4 is NULL");
    p->sigma_c = params4[0];
    p->sigma_z = params4[1];
    p->eps_a = params4[2];
    p->eps_z = params4[3];
    if (!positive_finite(p->sigma_c) || !positive_finite(p->sigma_z))
        return fail(PRT_ERR_ARG, who + ": sigma_c and sigma_z must be positive and finite");
    if (!positive_finite(p->eps_a) || !positive_finite(p->eps_z))
        return fail(PRT_ERR_ARG, who + ": eps_a and eps_z must be positive and finite");
    // the last pass divides by (sigma_c * 2^-i)^2: it must not underflow to 0 or overflow
    const float sc_last = p->sigma_c * (1.0f / (float)(1 << (iterations > 0 ? iterations - 1 : 0)));
    if (!positive_finite(sc_last * sc_last) || !positive_finite(p->sigma_c * p->sigma_c))
        return fail(PRT_ERR_ARG, who + ": sigma_c squared leaves the f32 range");
    return PRT_OK;
}

// check_args for the variance-guided entry points (params5 = sigma_l, sigma_z, eps_a, eps_z, eps_l)
int check_var_args(const char* fn, int device, int W, int H, int iterations, const float* params5,
                   prt_dn::VarParams* p) {
    const std::string who(fn);
    if (device < 0) return fail(PRT_ERR_ARG, who + ": device < 0");
    if (W < 1 || H < 1) return fail(PRT_ERR_ARG, who + ": W and H must be >= 1");
    if (W > prt_dn::kMaxSide || H > prt_dn::kMaxSide)
        return fail(PRT_ERR_ARG, who + ": W and H must be <= " + std::to_string(prt_dn::kMaxSide));
    if (iterations < 0 || iterations > prt_dn::kMaxIterations)
        return fail(PRT_ERR_ARG, who + ": iterations must be in 0.." + std::to_string(prt_dn::kMaxIterations));
    if (!params5) return fail(PRT_ERR_ARG, who + ": params5 is NULL");
    p->sigma_l = params5[0];
    p->sigma_z = params5[1];
    p->eps_a = params5[2];
    p->eps_z = params5[3];
    p->eps_l = params5[4];
    if (!positive_finite(p->sigma_l) || !positive_finite(p->sigma_z))
        return fail(PRT_ERR_ARG, who + ": sigma_l and sigma_z must be positive and finite");
    if (!positive_finite(p->eps_a) || !positive_finite(p->eps_z) || !positive_finite(p->eps_l))
        return fail(PRT_ERR_ARG, who + ": eps_a, eps_z and eps_l must be positive and finite");
    return PRT_OK;
}

// checks of the moments entry points; a frame_pitch of 0 (packed) is replaced by W * H * 3
int check_moments_args(const char* fn, int device, int n_frames, int64_t* frame_pitch, float n_samples, float eps_a,
                       int W, int H) {
    const std::string who(fn);
    if (device < 0) return fail(PRT_ERR_ARG, who + ": device < 0");
    if (W < 1 || H < 1) return fail(PRT_ERR_ARG, who + ": W and H must be >= 1");
    if (W > prt_dn::kMaxSide || H > prt_dn::kMaxSide)
        return fail(PRT_ERR_ARG, who + ": W and H must be <= " + std::to_string(prt_dn::kMaxSide));
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

}  // namespace

extern "C" {

const char* prt_denoise_last_error(void) { return g_dn_err.c_str(); }

int64_t prt_denoise_work_bytes(int W, int H) {
    if (W < 1 || H < 1 || W > prt_dn::kMaxSide || H > prt_dn::kMaxSide) return 0;
    return (int64_t)prt_dn::work_bytes(W, H);
}

int prt_denoise_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                       const float* params4, float* d_out, void* d_work, int64_t work_bytes, void* stream) {
    prt_dn::Params p;
    if (!d_color || !d_feat || !d_out || !d_work)
        return fail(PRT_ERR_ARG, "prt_denoise_device: NULL pointer");
    int rc = check_args("prt_denoise_device", device, W, H, iterations, params4, &p);
    if (rc != PRT_OK) return rc;
    if (work_bytes < (int64_t)prt_dn::work_bytes(W, H))
        return fail(PRT_ERR_ARG, "prt_denoise_device: d_work is smaller than prt_denoise_work_bytes(W, H)");
    if (reinterpret_cast<uintptr_t>(d_work) % 16 != 0)
        return fail(PRT_ERR_ARG, "prt_denoise_device: d_work must be 16-byte aligned");
    if (d_out == d_color) return fail(PRT_ERR_ARG, "prt_denoise_device: d_out must not alias d_color");
    rc = check_device("prt_denoise_device", device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    DN_HIP_TRY(prt_dn::enqueue(d_color, d_feat, W, H, iterations, p, d_out, d_work, static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_denoise(int device, const float* color, const float* feat, int W, int H, int iterations,
                const float* params4, float* out) {
    prt_dn::Params p;
    if (!color || !feat || !out) return fail(PRT_ERR_ARG, "prt_denoise: NULL pointer");
    int rc = check_args("prt_denoise", device, W, H, iterations, params4, &p);
    if (rc != PRT_OK) return rc;
    rc = check_device("prt_denoise", device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    const size_t n = (size_t)W * (size_t)H;
    DevMem d_color, d_feat, d_out, d_work;
    if (hipMalloc(&d_color.p, n * 3 * sizeof(float)) != hipSuccess || hipMalloc(&d_feat.p, n * 8 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d_out.p, n * 3 * sizeof(float)) != hipSuccess || hipMalloc(&d_work.p, prt_dn::work_bytes(W, H)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PRT_ERR_OOM, "prt_denoise: device allocation failed");
    }
    DN_HIP_TRY(hipMemcpy(d_color.p, color, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_feat.p, feat, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(prt_dn::enqueue(static_cast<const float*>(d_color.p), static_cast<const float*>(d_feat.p), W, H, iterations,
                               p, static_cast<float*>(d_out.p), d_work.p, nullptr));
    // the copy on the null stream follows the kernels and blocks until it is done
    DN_HIP_TRY(hipMemcpy(out, d_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PRT_OK;
}

int64_t prt_denoise_var_work_bytes(int W, int H) {
    if (W < 1 || H < 1 || W > prt_dn::kMaxSide || H > prt_dn::kMaxSide) return 0;
    return (int64_t)prt_dn::var_work_bytes(W, H);
}

int prt_denoise_var_device(int device, const float* d_color, const float* d_feat, int W, int H, int iterations,
                           const float* params5, float* d_out, float* d_out_var, void* d_work, int64_t work_bytes,
                           void* stream) {
    prt_dn::VarParams p;
    if (!d_color || !d_feat || !d_out || !d_work)
        return fail(PRT_ERR_ARG, "prt_denoise_var_device: NULL pointer");
    int rc = check_var_args("prt_denoise_var_device", device, W, H, iterations, params5, &p);
    if (rc != PRT_OK) return rc;
    if (work_bytes < (int64_t)prt_dn::var_work_bytes(W, H))
        return fail(PRT_ERR_ARG, "prt_denoise_var_device: d_work is smaller than prt_denoise_var_work_bytes(W, H)");
    if (reinterpret_cast<uintptr_t>(d_work) % 16 != 0)
        return fail(PRT_ERR_ARG, "prt_denoise_var_device: d_work must be 16-byte aligned");
    if (d_out == d_color) return fail(PRT_ERR_ARG, "prt_denoise_var_device: d_out must not alias d_color");
    if (d_out_var && (d_out_var == d_out || d_out_var == d_color || d_out_var == d_feat))
        return fail(PRT_ERR_ARG, "prt_denoise_var_device: d_out_var must not alias d_out, d_color or d_feat");
    rc = check_device("prt_denoise_var_device", device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    DN_HIP_TRY(prt_dn::enqueue_var(d_color, d_feat, W, H, iterations, p, d_out, d_out_var, d_work,
                                   static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_denoise_var(int device, const float* color, const float* feat, int W, int H, int iterations,
                    const float* params5, float* out, float* out_var) {
    prt_dn::VarParams p;
    if (!color || !feat || !out) return fail(PRT_ERR_ARG, "prt_denoise_var: NULL pointer");
    int rc = check_var_args("prt_denoise_var", device, W, H, iterations, params5, &p);
    if (rc != PRT_OK) return rc;
    rc = check_device("prt_denoise_var", device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    const size_t n = (size_t)W * (size_t)H;
    DevMem d_color, d_feat, d_out, d_var, d_work;
    if (hipMalloc(&d_color.p, n * 3 * sizeof(float)) != hipSuccess || hipMalloc(&d_feat.p, n * 8 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d_out.p, n * 3 * sizeof(float)) != hipSuccess || (out_var && hipMalloc(&d_var.p, n * sizeof(float)) != hipSuccess) ||
        hipMalloc(&d_work.p, prt_dn::var_work_bytes(W, H)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PRT_ERR_OOM, "prt_denoise_var: device allocation failed");
    }
    DN_HIP_TRY(hipMemcpy(d_color.p, color, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_feat.p, feat, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(prt_dn::enqueue_var(static_cast<const float*>(d_color.p), static_cast<const float*>(d_feat.p), W, H,
                                   iterations, p, static_cast<float*>(d_out.p), static_cast<float*>(d_var.p), d_work.p,
                                   nullptr));
    // the copies on the null stream follow the kernels and block until they are done
    DN_HIP_TRY(hipMemcpy(out, d_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) DN_HIP_TRY(hipMemcpy(out_var, d_var.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return PRT_OK;
}

// ---- variance from per-pixel sample moments ----

int prt_denoise_var_given_device(int device, const float* d_color, const float* d_feat, const float* d_in_var,
                                 int W, int H, int iterations, const float* params5, float* d_out,
                                 float* d_out_var, void* d_work, int64_t work_bytes, void* stream) {
    const char* fn = "prt_denoise_var_given_device";
    const std::string who(fn);
    prt_dn::VarParams p;
    if (!d_color || !d_feat || !d_in_var || !d_out || !d_work) return fail(PRT_ERR_ARG, who + ": NULL pointer");
    int rc = check_var_args(fn, device, W, H, iterations, params5, &p);
    if (rc != PRT_OK) return rc;
    if (work_bytes < (int64_t)prt_dn::var_work_bytes(W, H))
        return fail(PRT_ERR_ARG, who + ": d_work is smaller than prt_denoise_var_work_bytes(W, H)");
    if (reinterpret_cast<uintptr_t>(d_work) % 16 != 0) return fail(PRT_ERR_ARG, who + ": d_work must be 16-byte aligned");
    if (d_out == d_color) return fail(PRT_ERR_ARG, who + ": d_out must not alias d_color");
    if (d_out_var && (d_out_var == d_out || d_out_var == d_color || d_out_var == d_feat))
        return fail(PRT_ERR_ARG, who + ": d_out_var must not alias d_out, d_color or d_feat");
    if (d_in_var == d_out || d_in_var == d_out_var)
        return fail(PRT_ERR_ARG, who + ": d_in_var must not alias d_out or d_out_var");
    rc = check_device(fn, device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    DN_HIP_TRY(prt_dn::enqueue_var_given(d_color, d_feat, d_in_var, W, H, iterations, p, d_out, d_out_var, d_work,
                                         static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_denoise_var_given(int device, const float* color, const float* feat, const float* in_var, int W, int H,
                          int iterations, const float* params5, float* out, float* out_var) {
    const char* fn = "prt_denoise_var_given";
    prt_dn::VarParams p;
    if (!color || !feat || !in_var || !out) return fail(PRT_ERR_ARG, std::string(fn) + ": NULL pointer");
    int rc = check_var_args(fn, device, W, H, iterations, params5, &p);
    if (rc != PRT_OK) return rc;
    rc = check_device(fn, device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    const size_t n = (size_t)W * (size_t)H;
    DevMem d_color, d_feat, d_in, d_out, d_var, d_work;
    if (hipMalloc(&d_color.p, n * 3 * sizeof(float)) != hipSuccess || hipMalloc(&d_feat.p, n * 8 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d_in.p, n * sizeof(float)) != hipSuccess || hipMalloc(&d_out.p, n * 3 * sizeof(float)) != hipSuccess ||
        (out_var && hipMalloc(&d_var.p, n * sizeof(float)) != hipSuccess) ||
        hipMalloc(&d_work.p, prt_dn::var_work_bytes(W, H)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PRT_ERR_OOM, std::string(fn) + ": device allocation failed");
    }
    DN_HIP_TRY(hipMemcpy(d_color.p, color, n * 3 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_feat.p, feat, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_in.p, in_var, n * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(prt_dn::enqueue_var_given(static_cast<const float*>(d_color.p), static_cast<const float*>(d_feat.p),
                                         static_cast<const float*>(d_in.p), W, H, iterations, p,
                                         static_cast<float*>(d_out.p), static_cast<float*>(d_var.p), d_work.p, nullptr));
    // the copies on the null stream follow the kernels and block until they are done
    DN_HIP_TRY(hipMemcpy(out, d_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) DN_HIP_TRY(hipMemcpy(out_var, d_var.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return PRT_OK;
}

int prt_moments_add_device(int device, const float* d_sums, int n_frames, int64_t frame_pitch, float n_samples,
                           const float* d_feat, float eps_a, int W, int H, float* d_io_state, void* stream) {
    const char* fn = "prt_moments_add_device";
    if (!d_sums || !d_feat || !d_io_state) return fail(PRT_ERR_ARG, std::string(fn) + ": NULL pointer");
    int rc = check_moments_args(fn, device, n_frames, &frame_pitch, n_samples, eps_a, W, H);
    if (rc != PRT_OK) return rc;
    if (reinterpret_cast<uintptr_t>(d_io_state) % 16 != 0)
        return fail(PRT_ERR_ARG, std::string(fn) + ": d_io_state must be 16-byte aligned");
    rc = check_device(fn, device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    DN_HIP_TRY(prt_dn::enqueue_moments(d_sums, n_frames, (size_t)frame_pitch, n_samples, d_feat, eps_a, W, H, d_io_state,
                                       static_cast<hipStream_t>(stream)));
    return PRT_OK;
}

int prt_moments_add(int device, const float* sums, int n_frames, int64_t frame_pitch, float n_samples,
                    const float* feat, float eps_a, int W, int H, float* io_state) {
    const char* fn = "prt_moments_add";
    if (!sums || !feat || !io_state) return fail(PRT_ERR_ARG, std::string(fn) + ": NULL pointer");
    int rc = check_moments_args(fn, device, n_frames, &frame_pitch, n_samples, eps_a, W, H);
    if (rc != PRT_OK) return rc;
    rc = check_device(fn, device);
    if (rc != PRT_OK) return rc;
    DeviceGuard g(device);
    DN_HIP_TRY(g.err);
    const size_t n = (size_t)W * (size_t)H;
    // the frames as they lie in the caller's memory, gaps of a pitch included
    const size_t span = (size_t)(n_frames - 1) * (size_t)frame_pitch + n * 3;
    DevMem d_sums, d_feat, d_state;
    if (hipMalloc(&d_sums.p, span * sizeof(float)) != hipSuccess || hipMalloc(&d_feat.p, n * 8 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d_state.p, n * 4 * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PRT_ERR_OOM, std::string(fn) + ": device allocation failed");
    }
    DN_HIP_TRY(hipMemcpy(d_sums.p, sums, span * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_feat.p, feat, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(hipMemcpy(d_state.p, io_state, n * 4 * sizeof(float), hipMemcpyHostToDevice));
    DN_HIP_TRY(prt_dn::enqueue_moments(static_cast<const float*>(d_sums.p), n_frames, (size_t)frame_pitch, n_samples,
                                       static_cast<const float*>(d_feat.p), eps_a, W, H, static_cast<float*>(d_state.p),
                                       nullptr));
    // the copy on the null stream follows the kernel and blocks until it is done
    DN_HIP_TRY(hipMemcpy(io_state, d_state.p, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return PRT_OK;
}

}  // extern "C"

"""First-hit feature buffers and the edge-avoiding a-trous denoiser.

`features()` computes per-pixel albedo / shading normal / depth / hit fraction of the render's own
primary rays in one HIP kernel (prt_features; `features_device()` leaves them on the device);
`denoise()` runs the HIP filter of pyrenderer_amd/csrc/prt_denoise.hip (prt_denoise); `temporal_accumulate()`
carries a frame's integrated colour and luminance moments into the next camera (prt_temporal_accumulate), and
with `object_ids()` and `motion_rows()` across rigidly moving objects (prt_temporal_accumulate_motion).
There is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _native as N
from .device_scene import interleaved_tiles, unpack_tiles

# defaults chosen by tools/denoise_sweep.py (profiles/denoise_sweep.txt): the lowest
# geometric-mean RMSE ratio among the parameter sets that improve every frame of the sweep
ITERATIONS = 5
SIGMA_C = 0.25
SIGMA_Z = 1.0
EPS_A = 1e-2
EPS_Z = 1e-2

FEATURE_CHANNELS = 8
# rays per prt_camera_rays / prt_hit_all call of features_packed_host(): 2^20 rays are 32 MiB of rays and
# 64 MiB of hit records on the host, whatever the frame size
CHUNK_RAYS = 1 << 20
T_MIN, T_MAX = 1e-5, 99999.9   # the primary ray's range in PathTracer.trace (core/tracing.py:126-127)


def _slots_in_frame(W, H, tile, ids):
    """(n_tiles * tile * tile,) bool: slots (tile-major, then row ly, then column lx) whose pixel
    lies inside the W x H frame."""
    tx = (W + tile - 1) // tile
    ids = np.asarray(ids, np.int64)
    x = (ids % tx)[:, None, None] * tile + np.arange(tile)[None, None, :]
    y = (ids // tx)[:, None, None] * tile + np.arange(tile)[None, :, None]
    return ((x < W) & (y < H)).reshape(-1)


def features_packed(ds, cam_packed, W, H, *, samples=1, seed=0, tile=64, chunk_rays=CHUNK_RAYS):
    """features() for a DeviceScene and a packed camera record: one features_kernel launch
    (prt_features).  `tile` and `chunk_rays` are still accepted and no longer affect anything: the
    kernel owns one pixel per lane, with no tile slots and no per-ray buffers to chunk."""
    if int(samples) < 1:
        raise ValueError("samples must be >= 1")
    return ds.features(cam_packed, int(W), int(H), samples=int(samples), seed=seed)


def features_device(ds, cam_packed, W, H, d_out_ptr, *, samples=1, first_sample=0, seed=0, quantized=False,
                    stream_ptr=None):
    """prt_features_device: the same features into device memory at `d_out_ptr` (W x H x 8 float32, [x][y],
    16-byte aligned; e.g. a torch tensor's data_ptr()), enqueued on `stream_ptr` (a hipStream_t; None = the
    null stream) without a host synchronisation: the `d_feat_ptr` of denoise_device and its kin."""
    ds.features_device(cam_packed, int(W), int(H), d_out_ptr, samples=int(samples), first_sample=int(first_sample),
                       seed=seed, quantized=quantized, stream_ptr=stream_ptr)


def features_packed_host(ds, cam_packed, W, H, *, samples=1, seed=0, tile=64, chunk_rays=CHUNK_RAYS, first_sample=0):
    """The slow path, kept as the restatement the tests compare prt_features against: the same features
    composed on the host, per chunk of `chunk_rays` rays from prt_camera_rays, prt_hit_all and float32
    sums in sample order over samples first_sample .. first_sample + samples - 1 (what features_packed
    did before the kernel; DESIGN.md §11 has both times)."""
    W, H, tile, samples, first_sample = int(W), int(H), int(tile), int(samples), int(first_sample)
    if samples < 1:
        raise ValueError("samples must be >= 1")
    ids = interleaved_tiles(W, H, tile)
    per_tile = tile * tile
    group = max(1, chunk_rays // per_tile)
    n_f32 = np.float32(samples)
    feat = np.zeros((W, H, FEATURE_CHANNELS), np.float32)   # the only frame-sized array held
    for g0 in range(0, ids.shape[0], group):
        gid = ids[g0:g0 + group]
        n_slots = gid.shape[0] * per_tile
        inside = _slots_in_frame(W, H, tile, gid)
        n_in = int(inside.sum())
        acc = np.zeros((n_slots, 8), np.float32)   # albedo sum, normal sum, t sum, hits
        step = max(1, chunk_rays // n_slots)
        for s0 in range(0, samples, step):
            k = min(step, samples - s0)
            o, d, _ = ds.camera_rays(cam_packed, W, H, tile, tile, gid, first_sample + s0, k, seed)
            # slots of partial edge tiles outside the frame carry all-zero rays: they never reach the traversal
            keep = np.tile(inside, k)
            hits = ds.hit_all(o[keep], d[keep], T_MIN, T_MAX).reshape(k, n_in, 16)
            for j in range(k):   # float32 sums in sample order
                r = hits[j]
                hit = r[:, 0] > 0
                acc[inside, 0:3] += r[:, 9:12]
                acc[inside, 3:6] += r[:, 5:8]
                acc[inside, 6] += np.where(hit, r[:, 1], np.float32(0.0))
                acc[inside, 7] += hit.astype(np.float32)
        hits_sum = acc[:, 7].copy()
        acc[:, 0:6] /= n_f32
        acc[:, 6] /= np.maximum(hits_sum, np.float32(1.0))
        acc[:, 7] /= n_f32
        unpack_tiles(acc, W, H, tile, tile, gid, feat)
    return feat


def features(scene, camera, *, resolution=None, samples=1, seed=0, device=0, tile=64, world=None):
    """First-hit feature buffers, (W, H, 8) float32 indexed [x][y]: the per-pixel mean over samples
    0 .. samples-1 of the render's own primary rays (same seed, resolution and tile as the render).

    [0:3] albedo (bsdf.evaluate() at the first hit; misses add 0), [3:6] shading normal (flipped
    toward the ray; misses add 0), [6] depth (sum of t over the hitting samples / max(hits, 1)),
    [7] hit fraction (hits / samples).
    """
    from .core.tracing import _Frame
    f = _Frame.of(scene, camera, depth=0, seed=seed, resolution=resolution, devices=(device,), tile=tile, world=world)
    return features_packed(f.ds, f.cam, f.W, f.H, samples=samples, seed=seed, tile=tile)


def _frame_and_features(mean, feat):
    """`mean` (W, H, 3) and `feat` (W, H, 8) as C-contiguous float32 arrays, and W, H."""
    mean = np.ascontiguousarray(mean, np.float32)
    feat = np.ascontiguousarray(feat, np.float32)
    if mean.ndim != 3 or mean.shape[2] != 3:
        raise ValueError(f"mean must be (W, H, 3), not {mean.shape}")
    if feat.shape != mean.shape[:2] + (FEATURE_CHANNELS,):
        raise ValueError(f"feat must be {mean.shape[:2] + (FEATURE_CHANNELS,)}, not {feat.shape}")
    return mean, feat, mean.shape[0], mean.shape[1]


def _vp(address):
    """A device address as a ctypes pointer; None or 0 is NULL."""
    return ctypes.c_void_p(address) if address else None


def _params(sigma_c, sigma_z, eps_a, eps_z):
    return np.array([sigma_c, sigma_z, eps_a, eps_z], np.float32)


def denoise(mean, feat, *, iterations=ITERATIONS, sigma_c=SIGMA_C, sigma_z=SIGMA_Z, eps_a=EPS_A, eps_z=EPS_Z,
            device=0):
    """Filter the mean radiance `mean` (W, H, 3) guided by `feat` (W, H, 8) from features():
    `iterations` a-trous passes (0..8) on the GPU `device`; returns (W, H, 3) float32.

    sigma_c: colour edge-stopping width (in demodulated radiance, halved every pass); sigma_z: depth
    edge-stopping width relative to the local depth gradient; eps_a: albedo floor of the
    demodulation; eps_z: depth floor.  Pixels without a first hit, and pixels whose colour or
    features are not finite, are returned unchanged."""
    mean, feat, W, H = _frame_and_features(mean, feat)
    out = np.zeros_like(mean)
    par = _params(sigma_c, sigma_z, eps_a, eps_z)
    N.check_denoise(N.lib().prt_denoise(int(device), N.ptr(mean), N.ptr(feat), W, H, int(iterations), N.ptr(par),
                                        N.ptr(out)))
    return out


def work_bytes(W, H):
    """Scratch bytes denoise_device needs for a W x H frame."""
    return int(N.lib().prt_denoise_work_bytes(int(W), int(H)))


def denoise_device(d_color_ptr, d_feat_ptr, W, H, d_out_ptr, d_work_ptr, n_work_bytes, *, iterations=ITERATIONS,
                   sigma_c=SIGMA_C, sigma_z=SIGMA_Z, eps_a=EPS_A, eps_z=EPS_Z, device=0, stream_ptr=None):
    """prt_denoise_device: the same filter on device pointers (e.g. torch tensors' data_ptr()),
    enqueued on `stream_ptr` (a hipStream_t; None = the null stream) without a host synchronisation."""
    par = _params(sigma_c, sigma_z, eps_a, eps_z)
    N.check_denoise(N.lib().prt_denoise_device(int(device), _vp(d_color_ptr), _vp(d_feat_ptr), int(W), int(H),
                                               int(iterations), N.ptr(par), _vp(d_out_ptr), _vp(d_work_ptr),
                                               int(n_work_bytes), _vp(stream_ptr)))


# ---- variance-guided mode (prt_denoise_var) ----
# defaults chosen by tools/denoise_sweep.py --mode variance (profiles/denoise_var_sweep.txt) by the
# fixed filter's rule; eps_a and eps_z are the fixed filter's
VAR_SIGMA_L = 1.0
VAR_SIGMA_Z = 2.0
VAR_EPS_L = 1e-2
MODES = ("fixed", "variance")


VARIANCE_FALLBACKS = ("zero", "spatial")


def _params_variance(sigma_l, sigma_z, eps_a, eps_z, eps_l):
    return np.array([sigma_l, sigma_z, eps_a, eps_z, eps_l], np.float32)


def _check_fallback(variance_fallback, has_plane):
    if variance_fallback not in VARIANCE_FALLBACKS:
        raise ValueError(f"variance_fallback must be one of {VARIANCE_FALLBACKS}, not {variance_fallback!r}")
    if variance_fallback == "spatial" and not has_plane:
        raise ValueError("variance_fallback='spatial' needs a variance plane to fall back from")


def _variance_entry(has_plane, variance_fallback, form=""):
    """The variance-guided filter's entry point of `form` ("" or "_device"): prt_denoise_var without a
    variance plane, with one prt_denoise_var_mixed for the "spatial" fallback and prt_denoise_var_given else."""
    stem = "prt_denoise_var"
    if has_plane:
        stem += "_mixed" if variance_fallback == "spatial" else "_given"
    return getattr(N.lib(), stem + form)


def denoise_variance(mean, feat, *, iterations=ITERATIONS, sigma_l=VAR_SIGMA_L, sigma_z=VAR_SIGMA_Z, eps_a=EPS_A,
                     eps_z=EPS_Z, eps_l=VAR_EPS_L, device=0, return_variance=False, variance=None,
                     variance_fallback="zero"):
    """denoise() with the colour edge-stopping width taken from the image's own noise: a 7 x 7
    estimate of the variance of the demodulated luminance scales it per pixel, and the variance is
    carried through the passes.  Returns (W, H, 3) float32, or with return_variance=True the pair
    (image, (W, H) float32 variance estimate before any pass).

    sigma_l: luminance edge-stopping width in local standard deviations; eps_l: its floor, in
    demodulated radiance; sigma_z, eps_a, eps_z: as in denoise().

    variance: None (default) estimates the variance from the image as described.  A (W, H) plane, e.g.
    channel 3 of a moments state (moments_add), is used in its place (prt_denoise_var_given): at a pixel
    that is filtered a finite value >= 0 is taken as it is, anything else counts as 0.  The variance
    returned with return_variance=True is then the one actually used.

    variance_fallback: what stands where `variance` is not finite and >= 0.  "zero" (default) is the rule
    above.  "spatial" (prt_denoise_var_mixed) runs the 7 x 7 estimate too and keeps it there: the plane of a
    temporal state (temporal_accumulate) holds a NaN wherever its history is too short to trust."""
    _check_fallback(variance_fallback, variance is not None)
    mean, feat, W, H = _frame_and_features(mean, feat)
    out = np.zeros_like(mean)
    var = np.zeros((W, H), np.float32) if return_variance else None
    par = _params_variance(sigma_l, sigma_z, eps_a, eps_z, eps_l)
    given = []
    if variance is not None:
        plane = np.ascontiguousarray(variance, np.float32)
        if plane.shape != (W, H):
            raise ValueError(f"variance must be {(W, H)}, not {plane.shape}")
        given = [N.ptr(plane)]
    fn = _variance_entry(variance is not None, variance_fallback)
    N.check_denoise(fn(int(device), N.ptr(mean), N.ptr(feat), *given, W, H, int(iterations), N.ptr(par), N.ptr(out),
                       N.ptr(var)))
    return (out, var) if return_variance else out


def filtered(mean, feat, mode="fixed", *, variance=None, return_variance=False, **params):
    """The one choice of filter: denoise() in mode "fixed", denoise_variance() in mode "variance" (with
    `variance`, if given, in place of its spatial estimate); `params` are the filter's keyword parameters.
    return_variance=True returns the pair (image, variance used), None for the fixed filter, which has none."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, not {mode!r}")
    if mode == "variance":
        return denoise_variance(mean, feat, variance=variance, return_variance=return_variance, **params)
    if variance is not None:
        raise TypeError("variance is a parameter of mode 'variance'")
    out = denoise(mean, feat, **params)
    return (out, None) if return_variance else out


def work_bytes_variance(W, H):
    """Scratch bytes denoise_variance_device needs for a W x H frame."""
    return int(N.lib().prt_denoise_var_work_bytes(int(W), int(H)))


def denoise_variance_device(d_color_ptr, d_feat_ptr, W, H, d_out_ptr, d_work_ptr, n_work_bytes, *, d_out_var_ptr=None,
                            iterations=ITERATIONS, sigma_l=VAR_SIGMA_L, sigma_z=VAR_SIGMA_Z, eps_a=EPS_A, eps_z=EPS_Z,
                            eps_l=VAR_EPS_L, device=0, stream_ptr=None, d_in_var_ptr=None, variance_fallback="zero"):
    """prt_denoise_var_device: denoise_variance on device pointers, enqueued on `stream_ptr` without a
    host synchronisation; `d_out_var_ptr` (W x H floats, optional) receives the variance estimate.
    `d_in_var_ptr` (W x H floats, optional) is denoise_variance's `variance` (prt_denoise_var_given_device,
    same scratch); it must not alias the output or `d_out_var_ptr`.  variance_fallback="spatial" keeps the
    7 x 7 estimate where that plane is not finite and >= 0 (prt_denoise_var_mixed_device)."""
    _check_fallback(variance_fallback, bool(d_in_var_ptr))
    par = _params_variance(sigma_l, sigma_z, eps_a, eps_z, eps_l)
    fn = _variance_entry(bool(d_in_var_ptr), variance_fallback, "_device")
    given = [_vp(d_in_var_ptr)] if d_in_var_ptr else []
    N.check_denoise(fn(int(device), _vp(d_color_ptr), _vp(d_feat_ptr), *given, int(W), int(H), int(iterations),
                       N.ptr(par), _vp(d_out_ptr), _vp(d_out_var_ptr), _vp(d_work_ptr), int(n_work_bytes),
                       _vp(stream_ptr)))


# ---- variance from per-pixel sample moments (prt_moments_add, prt_denoise_var_given) ----
MOMENT_CHANNELS = 4          # k, mean, M2, var_mean
# batches a moments state must hold before Accumulator.denoised(mode="variance") trusts its variance
# (SVGF's history threshold); below it the spatial estimate is used
MIN_MOMENT_BATCHES = 4


def moments_state(W, H):
    """The empty moments state of a W x H frame: (W, H, 4) float32 zeros, [x][y]; channels k (batches
    seen), mean of the batches' demodulated luminance, M2, var_mean (the variance of that mean)."""
    return np.zeros((int(W), int(H), MOMENT_CHANNELS), np.float32)


def moments_add(state, sums_frames, n_samples, feat, *, eps_a=EPS_A, device=0):
    """Welford update of `state` (moments_state, modified in place and returned) with the batch frames
    `sums_frames`: (n_frames, W, H, 3) or (W, H, 3) per-pixel radiance SUMS, each over `n_samples`
    samples (the same count for every frame ever added to one state).  `feat`: (W, H, 8) features.
    state[..., 3] is the variance of the mean over all batches seen, 0 below two batches; its square
    root is the standard error of the demodulated luminance."""
    if not (isinstance(state, np.ndarray) and state.dtype == np.float32 and state.flags.c_contiguous
            and state.ndim == 3 and state.shape[2] == MOMENT_CHANNELS):
        raise ValueError("state must be a C-contiguous float32 (W, H, 4) array (moments_state)")
    W, H = state.shape[:2]
    frames = np.ascontiguousarray(sums_frames, np.float32)
    if frames.ndim == 3:
        frames = frames[None]
    if frames.ndim != 4 or frames.shape[1:] != (W, H, 3) or frames.shape[0] < 1:
        raise ValueError(f"sums_frames must be (n_frames, {W}, {H}, 3) or ({W}, {H}, 3), not {frames.shape}")
    feat = np.ascontiguousarray(feat, np.float32)
    if feat.shape != (W, H, FEATURE_CHANNELS):
        raise ValueError(f"feat must be {(W, H, FEATURE_CHANNELS)}, not {feat.shape}")
    N.check_denoise(N.lib().prt_moments_add(int(device), N.ptr(frames), frames.shape[0], 0, float(n_samples),
                                            N.ptr(feat), float(eps_a), W, H, N.ptr(state)))
    return state


def moments_add_device(d_sums_ptr, n_frames, n_samples, d_feat_ptr, W, H, d_state_ptr, *, frame_pitch=0, eps_a=EPS_A,
                       device=0, stream_ptr=None):
    """prt_moments_add_device: moments_add on device pointers, enqueued on `stream_ptr` without a host
    synchronisation.  Frame f starts at d_sums_ptr + f * frame_pitch floats (0 = packed); the state
    (W x H x 4 floats, 16-byte aligned) is updated in place."""
    N.check_denoise(N.lib().prt_moments_add_device(int(device), _vp(d_sums_ptr), int(n_frames), int(frame_pitch),
                                                   float(n_samples), _vp(d_feat_ptr), float(eps_a), int(W), int(H),
                                                   _vp(d_state_ptr), _vp(stream_ptr)))


# ---- temporal accumulation (prt_temporal_accumulate; DESIGN.md §11 "Temporal accumulation") ----
TEMPORAL_CHANNELS = 8        # I.rgb, h, m1, m2, var, 0
# alpha (= alpha_m), tau_z and tau_n chosen by tools/denoise_sweep.py --mode temporal
# (profiles/denoise_temporal_sweep.txt) by the filters' rule: the lowest geometric-mean RMSE ratio among the sets
# that leave no sequence worse than the variance-guided filter alone (tau_n 0.8 and 0.9 tie; the stricter one
# stands).  tau_a, min_history and w_min were not swept; eps_a is the filters'
TEMPORAL_ALPHA = 0.2         # floor of the colour's blend weight: 1 / alpha frames of effective history
TEMPORAL_ALPHA_M = 0.2       # ... of the luminance moments'
TEMPORAL_TAU_N = 0.9         # least dot product of the two shading normals
TEMPORAL_TAU_Z = 0.05        # greatest relative difference of the reprojected distance
TEMPORAL_TAU_A = 0.05        # greatest difference of an albedo channel
TEMPORAL_MIN_HISTORY = 4.0   # frames before the temporal variance is trusted (SVGF's threshold)
TEMPORAL_W_MIN = 0.25        # least sum of accepted bilinear weights
TEMPORAL_PARAMS = ("alpha", "alpha_m", "tau_n", "tau_z", "tau_a", "eps_a", "min_history", "w_min")


def _params_temporal(alpha, alpha_m, tau_n, tau_z, tau_a, eps_a, min_history, w_min):
    return np.array([alpha, alpha_m, tau_n, tau_z, tau_a, eps_a, min_history, w_min], np.float32)


def _camera_record(cam, name):
    cam = np.ascontiguousarray(cam, np.float32)
    if cam.shape != (24,):
        raise ValueError(f"{name} must be a packed camera record of 24 floats, not {cam.shape}")
    if cam[19] > 0:
        raise ValueError(f"{name} has an aperture: a thin lens has no unique reprojection")
    return cam


def temporal_state(W, H):
    """A (W, H, 8) float32 array of zeros for a temporal state, [x][y]: channels I.rgb (integrated
    demodulated colour), h (history length), m1, m2 (integrated luminance moments), the variance plane, 0."""
    return np.zeros((int(W), int(H), TEMPORAL_CHANNELS), np.float32)


IDENTITY_ROW = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
MAX_OBJECTS = 1 << 20        # prt_temporal_accumulate_motion's limit on the motion table
RIGID_TOL = 1e-9             # float64 bound on |R^T R - 1| (per entry) and |det R - 1| of a rigid motion


def object_ids(ds, cam_packed, W, H):
    """The object-id plane of a frame, (W, H) int32 [x][y]: the index in scene.primitives of the closest hit of
    the pixel-centre ray PackedCamera.gen_ray((x + 0.5) / (W - 1), (y + 0.5) / (H - 1)), the one temporal_kernel
    restates, in T_MIN..T_MAX; -1 at a miss.  Composed through the host from ds.closest_hits, flat.tri_prim and
    flat.sph_prim (one ray record up and one hit id down per pixel; DESIGN.md §11 has the cost).  With W == 1
    or H == 1 no pixel-centre ray exists: all -1, and nothing is traced."""
    from .core.camera import PackedCamera
    W, H = int(W), int(H)
    ids = np.full((W, H), -1, np.int32)
    if W == 1 or H == 1:
        return ids
    f = np.float32
    u = (np.arange(W, dtype=f) + f(0.5)) / f(W - 1)
    v = (np.arange(H, dtype=f) + f(0.5)) / f(H - 1)
    o, d = PackedCamera.from_record(cam_packed).gen_ray(u[:, None], v[None, :])
    flat = ds.flat
    for x0 in range(0, W, max(1, CHUNK_RAYS // H)):
        x1 = min(W, x0 + max(1, CHUNK_RAYS // H))
        hid, _ = ds.closest_hits(o[x0:x1].reshape(-1, 3), d[x0:x1].reshape(-1, 3), T_MIN, T_MAX)
        hid = hid.astype(np.int64)
        tri, sph = (hid >= 0) & (hid < flat.n_tri), hid >= flat.n_tri
        out = np.full(hid.shape, -1, np.int32)
        out[tri] = flat.tri_prim[hid[tri]]
        out[sph] = flat.sph_prim[hid[sph] - flat.n_tri]
        ids[x0:x1] = out.reshape(x1 - x0, H)
    return ids


def _same_primitive(a, b):
    if type(a) is not type(b) or getattr(a, "type_name", "") != getattr(b, "type_name", ""):
        return False
    if hasattr(a, "faces") != hasattr(b, "faces") or (hasattr(a, "faces") and len(a.faces) != len(b.faces)):
        return False
    return a.bsdf is b.bsdf or np.array_equal(a.bsdf.pack(), b.bsdf.pack())


def motion_rows(prev_scene, scene):
    """The motion table of a frame, (n_primitives, 12) float32: per primitive of `scene` the row-major 3 x 4
    matrix that takes a world position of this frame to the same material point's position in `prev_scene`.
    The two scenes must list the same primitives in the same order (type, face count, BSDF); anything else is a
    ValueError.  Mesh primitives: T_prev @ inv(T_cur) in float64 from trans_mat; spheres: the translation of the
    centre.  A primitive whose transform did not change gets the exact identity row, not a computed one.  A
    pair that is not rigid (the 3 x 3 part not orthonormal with determinant +1 within RIGID_TOL in float64, a
    singular transform, a sphere whose radius changed) or that has no transform to compare (a MeshBatch whose
    vertices changed) gets a NaN row: "no previous pose", its pixels start afresh."""
    a, b = list(prev_scene.primitives), list(scene.primitives)
    if len(a) != len(b):
        raise ValueError(f"the scenes list {len(a)} and {len(b)} primitives: motion needs the same primitives in "
                         f"the same order")
    rows = np.tile(IDENTITY_ROW, (len(b), 1))
    for i, (p, c) in enumerate(zip(a, b)):
        if not _same_primitive(p, c):
            raise ValueError(f"primitive {i} differs between the scenes (type, face count or BSDF): motion needs "
                             f"the same primitives in the same order")
        if getattr(c, "type_name", "") == "sphere":
            if p.radius != c.radius:
                rows[i] = np.nan
            elif not np.array_equal(p.center, c.center):
                rows[i, [3, 7, 11]] = np.asarray(p.center, np.float64) - np.asarray(c.center, np.float64)
            continue
        if not hasattr(c, "trans_mat"):
            if not np.array_equal(p.vertices, c.vertices):
                rows[i] = np.nan
            continue
        tp, tc = np.asarray(p.trans_mat, np.float64), np.asarray(c.trans_mat, np.float64)
        if np.array_equal(tp, tc):
            continue
        try:
            m = tp @ np.linalg.inv(tc)
        except np.linalg.LinAlgError:
            rows[i] = np.nan
            continue
        r = m[:3, :3]
        rigid = (np.isfinite(m).all() and np.abs(r.T @ r - np.eye(3)).max() <= RIGID_TOL
                 and abs(np.linalg.det(r) - 1.0) <= RIGID_TOL)
        rows[i] = m[:3].reshape(12) if rigid else np.nan
    return rows.astype(np.float32)


def _motion_args(ids, motion, W, H):
    """(ids, motion, n_objects) of a call with per-object motion, as contiguous arrays."""
    if motion is None:
        raise ValueError("ids need a motion table: motion=(n_objects, 12) float32 rows (motion_rows), which may be empty")
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.shape != (W, H):
        raise ValueError(f"ids must be {(W, H)}, not {ids.shape}")
    motion = np.ascontiguousarray(motion, np.float32)
    if motion.ndim != 2 or motion.shape[1] != 12:
        raise ValueError(f"motion must be (n_objects, 12), not {motion.shape}")
    if motion.shape[0] > MAX_OBJECTS:
        raise ValueError(f"motion holds {motion.shape[0]} rows, more than {MAX_OBJECTS}")
    return ids, motion, motion.shape[0]


def _temporal_entry(moving, form=""):
    """The temporal entry point of `form` ("" or "_device"): prt_temporal_accumulate for the static world,
    prt_temporal_accumulate_motion with an id plane."""
    return getattr(N.lib(), "prt_temporal_accumulate" + ("_motion" if moving else "") + form)


def _temporal_call(form, device, frame, prev, motion, W, H, par, outs):
    """The one argument list of the four entry points.  frame = (colour, features, camera record) and prev =
    (features, camera record, state) as pointers; motion = (ids, prev ids, table, n_objects) or None for the
    static world; outs = (state, colour, variance), then the stream in the device form."""
    N.check_denoise(_temporal_entry(motion is not None, form)(int(device), *frame, *prev, *(motion or ()), int(W), int(H),
                                                               N.ptr(par), *outs))


def temporal_accumulate(mean, feat, cam, prev=None, *, alpha=TEMPORAL_ALPHA, alpha_m=TEMPORAL_ALPHA_M,
                        tau_n=TEMPORAL_TAU_N, tau_z=TEMPORAL_TAU_Z, tau_a=TEMPORAL_TAU_A, eps_a=EPS_A,
                        min_history=TEMPORAL_MIN_HISTORY, w_min=TEMPORAL_W_MIN, device=0, return_color=True,
                        ids=None, motion=None):
    """One frame of temporal accumulation.  `mean` (W, H, 3), `feat` (W, H, 8) and `cam` (the packed 24-float
    record) are this frame's; prev = (state, feat, cam) is the previous frame's, None on the first.  The
    previous state is reprojected through this frame's first hits into the previous camera, tested for
    consistency (normal, depth, albedo) and blended with this frame.  Returns (state, colour): the new
    (W, H, 8) state and the integrated colour (W, H, 3), re-modulated; just the state with
    return_color=False.  state[..., 3] is the history length, state[..., 6] the variance of the integrated
    luminance, NaN where the history is shorter than min_history: denoise_variance(colour, feat,
    variance=state[..., 6], variance_fallback="spatial") filters the result.

    ids, motion: None (default) is the static world above (prt_temporal_accumulate).  With `ids` (W, H) int32
    (object_ids) and `motion` (n_objects, 12) float32 (motion_rows), prev is (state, feat, cam, ids) and the
    history follows moving objects (prt_temporal_accumulate_motion): a pixel whose id has a row is carried by
    it into the previous frame's world before it is projected, and a tap counts only where the previous id
    equals the pixel's."""
    mean, feat, W, H = _frame_and_features(mean, feat)
    cam = _camera_record(cam, "cam")
    par = _params_temporal(alpha, alpha_m, tau_n, tau_z, tau_a, eps_a, min_history, w_min)
    moving = ids is not None
    if motion is not None and not moving:
        raise ValueError("a motion table needs the frame's ids (object_ids)")
    if moving:
        ids, motion, n_objects = _motion_args(ids, motion, W, H)
    p_state = p_feat = p_cam = p_ids = None
    if prev is not None:
        if len(prev) != (4 if moving else 3):
            raise ValueError("prev must be (state, feat, cam, ids) with ids and (state, feat, cam) without, not "
                             f"{len(prev)} items")
        p_state, p_feat, p_cam = prev[:3]
        p_state = np.ascontiguousarray(p_state, np.float32)
        p_feat = np.ascontiguousarray(p_feat, np.float32)
        if p_state.shape != (W, H, TEMPORAL_CHANNELS) or p_feat.shape != (W, H, FEATURE_CHANNELS):
            raise ValueError(f"prev must hold a {(W, H, TEMPORAL_CHANNELS)} state and {(W, H, FEATURE_CHANNELS)} "
                             f"features (the resolution cannot change), not {p_state.shape} and {p_feat.shape}")
        p_cam = _camera_record(p_cam, "prev's camera")
        if moving:
            p_ids = np.ascontiguousarray(prev[3], np.int32)
            if p_ids.shape != (W, H):
                raise ValueError(f"prev's ids must be {(W, H)}, not {p_ids.shape}")
    state = temporal_state(W, H)
    color = np.zeros_like(mean) if return_color else None
    table = (N.ptr(ids), N.ptr(p_ids), N.ptr(motion) if n_objects else None, n_objects) if moving else None
    _temporal_call("", device, (N.ptr(mean), N.ptr(feat), N.ptr(cam)), (N.ptr(p_feat), N.ptr(p_cam), N.ptr(p_state)),
                   table, W, H, par, (N.ptr(state), N.ptr(color), None))
    return (state, color) if return_color else state


def temporal_accumulate_device(d_color_ptr, d_feat_ptr, cam, W, H, d_state_ptr, *, d_prev_feat_ptr=None, prev_cam=None,
                               d_prev_state_ptr=None, d_out_color_ptr=None, d_out_var_ptr=None, alpha=TEMPORAL_ALPHA,
                               alpha_m=TEMPORAL_ALPHA_M, tau_n=TEMPORAL_TAU_N, tau_z=TEMPORAL_TAU_Z,
                               tau_a=TEMPORAL_TAU_A, eps_a=EPS_A, min_history=TEMPORAL_MIN_HISTORY,
                               w_min=TEMPORAL_W_MIN, device=0, stream_ptr=None, d_ids_ptr=None, d_prev_ids_ptr=None,
                               d_motion_ptr=None, n_objects=None):
    """prt_temporal_accumulate_device: temporal_accumulate on device pointers, enqueued on `stream_ptr` without
    a host synchronisation.  `cam` and `prev_cam` are host records; the state planes (W x H x 8 floats) must
    be 16-byte aligned and distinct; `d_out_var_ptr` (W x H floats) receives the variance plane, the
    `d_in_var_ptr` of denoise_variance_device(..., variance_fallback="spatial").

    With `d_ids_ptr` (W x H int32) the call is prt_temporal_accumulate_motion_device: `d_prev_ids_ptr` goes with
    the other previous planes, `d_motion_ptr` is the device table of `n_objects` rows of 12 floats (it may be
    None only with n_objects=0)."""
    cam = _camera_record(cam, "cam")
    p_cam = None if prev_cam is None else _camera_record(prev_cam, "prev_cam")
    par = _params_temporal(alpha, alpha_m, tau_n, tau_z, tau_a, eps_a, min_history, w_min)
    table = None
    if d_ids_ptr:
        if n_objects is None:
            raise ValueError("ids need a motion table: n_objects (which may be 0) and d_motion_ptr")
        table = (_vp(d_ids_ptr), _vp(d_prev_ids_ptr), _vp(d_motion_ptr), int(n_objects))
    elif d_prev_ids_ptr or d_motion_ptr or n_objects is not None:
        raise ValueError("d_prev_ids_ptr, d_motion_ptr and n_objects need the frame's d_ids_ptr")
    _temporal_call("_device", device, (_vp(d_color_ptr), _vp(d_feat_ptr), N.ptr(cam)),
                   (_vp(d_prev_feat_ptr), N.ptr(p_cam), _vp(d_prev_state_ptr)), table, W, H, par,
                   (_vp(d_state_ptr), _vp(d_out_color_ptr), _vp(d_out_var_ptr), _vp(stream_ptr)))

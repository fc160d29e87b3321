"""Path tracing entry points (reference: core/tracing.py:47-155, main_taichi.py:80-127).

`render(scene, camera, spp=..., depth=...)` is the build's `core.tracing.render()`
(named by BASELINE.json's north star; the reference has only the Taichi
`render()` closure of main_taichi.py:80-99).  It returns the MEAN linear
radiance per pixel — `pixels / samples` of main_taichi.py:61-64 before the
sqrt tone map — as float32 (W, H, 3) indexed [x][y] with y up, like the
reference's `pixels.to_numpy()`.  Every sample runs PathTracer.trace's
estimator in the HIP kernel (pyrenderer_amd/csrc/prt_kernels.hip).

`devices=(0, 1, ...)` shards 64x64 tiles across GPUs of this process
('latin' interleave, device_scene.tile_owner) through prt_render_multi, which
gathers the tile sums to the first device with one RCCL send/recv group; the
image is bit-identical for any device count since random numbers are keyed by
(seed, global pixel, sample).  For one process per GPU use
pyrenderer_amd.distributed (torch.distributed gather over RCCL/xGMI).

`Accumulator` is the progressive form of main_taichi.py:108-127 (render() once
per GUI frame, pixels += L, samples += 1, finish() of the running mean), with
save / load to resume an accumulation.

`TemporalAccumulator` / `render_sequence` render a camera path and carry the history across camera
moves (pyrenderer_amd.denoise.temporal_accumulate, DESIGN.md §11 "Temporal accumulation").

`render_adaptive` renders in batches and stops the tiles whose noise has reached a target
(pyrenderer_amd.adaptive.AdaptiveAccumulator); that module is imported only there.
"""
import hashlib
import os

import numpy as np

from ..device_scene import interleaved_tiles, render_multi, unpack_tiles
from ..mathematics.intersection import World


class PathTracer:
    """Same constructor as the reference (core/tracing.py:47-50).  `trace` runs the reference's
    per-ray estimator for a batch of caller rays; `render_sums` / `render` run render()'s
    per-pixel sample loop (main_taichi.py:80-99) over the whole frame."""

    def __init__(self, world, depth, img_w, img_h):
        self.world = world
        self.depth = depth
        self.img_w = img_w
        self.img_h = img_h

    def trace(self, ro, rd, depth=None, x=None, y=None, *, seed=0, device=0, nee="reference"):
        """PathTracer.trace (core/tracing.py:116-155) on the GPU: the radiance of one path per ray,
        for one ray ((3,) arrays) or a batch ((n, 3) arrays), as float32 (3,) / (n, 3).

        depth defaults to the constructor's.  x, y are accepted for the reference's signature
        (its trace ignores them).  Ray i draws from the random stream keyed (seed, i, 0): the
        streams render() uses minus the two camera-jitter draws (include/prt.h prt_trace_rays)."""
        o = np.asarray(ro, np.float32)
        single = o.ndim == 1
        ds = self.world.device_scene(device)
        out = ds.trace_rays(o, rd, self.depth if depth is None else int(depth), seed=seed, flags=nee_flags(nee))
        return out[0] if single else out

    def render_sums(self, cam_packed, spp, seed=0, devices=(0,), tile=64, flags=0):
        """Per-pixel radiance SUMS over spp samples, (W, H, 3) [x][y]."""
        return _Frame(self.world, cam_packed, self.img_w, self.img_h, depth=self.depth, seed=seed, devices=devices,
                      tile=tile, flags=flags).sums(spp)

    def render(self, cam_packed, spp, seed=0, devices=(0,), tile=64, nee="reference"):
        return _mean(self.render_sums(cam_packed, spp, seed, devices, tile, nee_flags(nee)), spp)


def nee_flags(nee):
    """Direct-lighting estimator: 'reference' = sample_direct_lighting, the one the
    reference's trace calls (core/tracing.py:92-108, :150-151); 'mis' = its unused MIS
    alternative sample_direct_lighting2 (core/tracing.py:57-90) in the same place."""
    from .._native import PRT_FLAG_MIS_NEE
    if nee == "reference":
        return 0
    if nee == "mis":
        return PRT_FLAG_MIS_NEE
    raise ValueError(f"nee must be 'reference' or 'mis', not {nee!r}")


def build_world(scene, devices=(0,)):
    world = World()
    for p in scene.primitives:
        world.add(p)
    return world.commit(devices)


def _check_variance_batches(variance_batches, spp, denoise, devices):
    """The rules for variance_batches, render()'s and the command line's; returns K (0 = off).  spp None:
    the caller's own passes are the batches (progressive rendering), K only switches the moments on."""
    if isinstance(variance_batches, (bool, np.bool_)) or not isinstance(variance_batches, (int, np.integer)):
        raise ValueError(f"variance_batches must be an integer, not {variance_batches!r}")
    K = int(variance_batches)
    if K == 0:
        return 0
    if K < 2:
        raise ValueError(f"variance_batches must be 0 or >= 2, not {K}")
    if not (isinstance(denoise, str) and denoise == "variance"):
        raise ValueError("variance_batches is a variance source of denoise='variance'")
    if spp is not None and (spp < K or spp % K):
        raise ValueError(f"spp ({spp}) must be a positive multiple of variance_batches ({K})")
    if len(tuple(devices)) != 1:
        raise ValueError("variance_batches renders on one device (prt_render_multi has no first-sample argument)")
    return K


def _mean(sums, spp):
    """pixels / samples (main_taichi.py:61-64, before the sqrt tone map); zeros without samples."""
    return sums / np.float32(spp) if spp > 0 else np.zeros_like(sums)


class _Frame:
    """What every entry point sets up once and the steps they share: the frame size, the world, the packed
    camera, the tile ids, the estimator flags and the devices.  The first of `devices` serves batches,
    features and the filter; all of them serve sums()."""

    def __init__(self, world, cam, W, H, *, depth, seed=0, devices=(0,), tile=64, flags=0):
        self.world, self.cam, self.W, self.H = world, cam, int(W), int(H)
        self.depth, self.seed, self.tile, self.flags = int(depth), int(seed), int(tile), flags
        self.devices = tuple(devices)
        self.device = self.devices[0]
        self.ids = interleaved_tiles(self.W, self.H, self.tile)
        self._feat = None

    @classmethod
    def of(cls, scene, camera, *, depth, seed=0, resolution=None, devices=(0,), tile=64, world=None, nee="reference"):
        """The frame of a scene and a camera; the world is built only if none is given."""
        W, H = resolution if resolution is not None else camera.resolution
        return cls(world or build_world(scene, devices), camera.convert_to_taichi_camera().packed(), W, H,
                   depth=depth, seed=seed, devices=devices, tile=tile, flags=nee_flags(nee))

    @property
    def ds(self):
        return self.world.device_scene(self.device)

    def zero_slots(self):
        return np.zeros((self.ids.shape[0] * self.tile * self.tile, 3), np.float32)

    def unpack(self, slots, frame=None):
        return unpack_tiles(slots, self.W, self.H, self.tile, self.tile, self.ids, frame)

    def sums(self, spp):
        """Radiance sums (W, H, 3) over samples 0 .. spp - 1, added in sample order on the device(s);
        zeros, without a render, for spp <= 0."""
        W, H, t = self.W, self.H, self.tile
        if spp <= 0:
            return np.zeros((W, H, 3), np.float32)
        if len(self.devices) > 1:
            return render_multi([self.world.device_scene(d) for d in self.devices], self.cam, W, H, t, spp,
                                self.depth, self.seed, self.flags)
        slots, _ = self.ds.render_tiles(self.cam, W, H, t, t, self.ids, spp, self.depth, self.seed, self.flags)
        return self.unpack(slots)

    def add_samples(self, first_sample, spp, onto=None, ids=None):
        """Samples first_sample .. first_sample + spp - 1 added in sample order onto the slot sums `onto`
        (modified in place and returned); by default onto zero sums, which makes them one batch.  ids: the
        tiles to render, in the slots' order (default: every tile of the frame)."""
        t, ids = self.tile, self.ids if ids is None else np.ascontiguousarray(ids, np.int32)
        slots = np.zeros((ids.shape[0] * t * t, 3), np.float32) if onto is None else onto
        return self.ds.render_tiles_accumulate(self.cam, self.W, self.H, t, t, ids, first_sample, spp,
                                               self.depth, slots, self.seed, self.flags)

    def batches(self, spp, K):
        """render_batches(): (sums, feat, state) of spp samples as K batches of spp / K."""
        from .. import denoise as D
        n = spp // K
        feat = self.features()
        frames = np.zeros((K, self.W, self.H, 3), np.float32)
        total = self.zero_slots()
        for j in range(K):
            batch = self.add_samples(j * n, n)
            total += batch
            self.unpack(batch, frames[j])
        state = D.moments_add(D.moments_state(self.W, self.H), frames, n, feat, device=self.device)
        return self.unpack(total), feat, state

    def features(self):
        """One-sample first-hit features of the frame's camera, seed and resolution, composed once and kept."""
        if self._feat is None:
            from .. import denoise as D
            self._feat = D.features_packed(self.ds, self.cam, self.W, self.H, samples=1, seed=self.seed,
                                           tile=self.tile)
        return self._feat

    def filter(self, mean, mode="fixed", **params):
        """`mean` filtered by pyrenderer_amd.denoise.filtered in `mode`, guided by features()."""
        from .. import denoise as D
        return D.filtered(mean, self.features(), mode, device=self.device, **params)


def render_batches(scene, camera, *, spp, depth, variance_batches, seed=0, resolution=None, device=0, tile=64,
                   world=None, nee="reference"):
    """spp samples as K = variance_batches batches of spp / K, with the per-pixel moments of the batch
    means: (sums (W, H, 3), feat (W, H, 8), state (W, H, 4)).  Batch j holds samples j * spp / K ..., each
    rendered from zero sums; `sums` adds the batch sums in batch order on the host, an association that
    differs in the last bits from render_sums()'s sample-order sum.  `feat` are the one-sample features
    render(denoise=...) uses and `state` is pyrenderer_amd.denoise.moments_add's over the K batches."""
    K = _check_variance_batches(variance_batches, spp, "variance", (device,))
    if K == 0:
        raise ValueError("variance_batches must be >= 2")
    return _Frame.of(scene, camera, depth=depth, seed=seed, resolution=resolution, devices=(device,), tile=tile,
                     world=world, nee=nee).batches(spp, K)


def render(scene, camera, *, spp, depth, seed=0, resolution=None, devices=(0,), tile=64, world=None,
           nee="reference", denoise=False, variance_batches=0):
    """Mean linear radiance (W, H, 3) float32, [x][y], y up.

    denoise: False (default) returns the Monte-Carlo mean as it is.  True filters it with the
    a-trous denoiser (pyrenderer_amd.denoise, default parameters) guided by one-sample first-hit
    features of the same camera, seed and resolution, on the first of `devices`.  "variance" selects
    its variance-guided mode (pyrenderer_amd.denoise.denoise_variance, default parameters), which
    takes the colour edge-stopping width from the image's own noise.  Anything else is a ValueError.

    variance_batches: 0 (default) is the path above exactly.  K >= 2, with denoise="variance", one device
    and spp a multiple of K, renders the spp samples as K batches of spp / K (render_batches) and gives
    the filter the variance of the mean measured from the K batch means per pixel
    (pyrenderer_amd.denoise.moments_add) in place of its 7 x 7 spatial estimate.  The unfiltered mean is
    then (sum of the batch sums, in batch order) / spp, which differs in the last bits from the
    sample-order sum of variance_batches=0.  Any other combination is a ValueError.

    nee: 'reference' (sample_direct_lighting, what the reference's trace runs) or 'mis'
    (the reference's unused MIS estimator sample_direct_lighting2, as an optional variant).

    resolution: (W, H) override of camera.resolution (the aspect ratio still
    comes from camera.resolution, as convert_to_taichi_camera() does).
    """
    if not (isinstance(denoise, (bool, np.bool_)) or (isinstance(denoise, str) and denoise == "variance")):
        raise ValueError(f"denoise must be False, True or 'variance', not {denoise!r}")
    K = _check_variance_batches(variance_batches, spp, denoise, devices)
    frame = _Frame.of(scene, camera, depth=depth, seed=seed, resolution=resolution, devices=devices, tile=tile,
                      world=world, nee=nee)
    if K:
        sums, _, state = frame.batches(spp, K)
        return frame.filter(_mean(sums, spp), "variance", variance=state[..., 3])
    mean = _mean(frame.sums(spp), spp)
    if not denoise:
        return mean
    return frame.filter(mean, "variance" if isinstance(denoise, str) else "fixed")


def render_sums(scene, camera, *, spp, depth, seed=0, resolution=None, devices=(0,), tile=64, world=None,
                nee="reference"):
    """Per-pixel radiance SUMS (W, H, 3) float32 [x][y] over spp samples — the reference's `pixels`
    field after spp render() passes (main_taichi.py:97); render() returns these / spp."""
    return _Frame.of(scene, camera, depth=depth, seed=seed, resolution=resolution, devices=devices, tile=tile,
                     world=world, nee=nee).sums(spp)


class Accumulator:
    """Progressive rendering on one device (main_taichi.py:108-127).

    `add(spp)` renders the next `spp` samples of every pixel and adds them in sample
    order onto the running per-pixel sums, so any split of N samples over add() calls
    leaves the sums bit-identical to `render(spp=N)` * N.  `mean()` is
    pixels / samples (main_taichi.py:61-64, before the sqrt tone map).  `save(path)` /
    `Accumulator.load(path, scene, camera)` resume an accumulation (.npz: sums, sample
    count, seed, depth, resolution, tile, estimator flags, the packed camera and a
    fingerprint of the flattened scene — load() refuses a different camera or scene,
    whose samples would otherwise be averaged into the same image).

    moments=True also keeps the per-pixel moments of the batch means (pyrenderer_amd.denoise.moments_add):
    every add(spp) is one batch, rendered from zero sums, added onto the running sums on the host (so the
    sums are the batch sums in batch order, which differs in the last bits from the sample-order sum
    above) and folded into the moments state.  Every batch must have the first batch's spp.
    denoised(mode="variance") then takes its variance from the state once it holds
    pyrenderer_amd.denoise.MIN_MOMENT_BATCHES batches, noise_map() is the per-pixel standard error, and
    save / load carry the state.  moments=False (default) leaves every bit and every saved field as above.
    """

    def __init__(self, scene, camera, *, depth, seed=0, resolution=None, device=0, tile=64, world=None,
                 nee="reference", moments=False):
        self.frame = _Frame.of(scene, camera, depth=depth, seed=seed, resolution=resolution, devices=(device,),
                               tile=tile, world=world, nee=nee)
        self.slots = self.frame.zero_slots()
        self.samples = 0
        self.moments = bool(moments)
        self.batch_spp = 0        # moments: the spp of every batch, 0 before the first
        self.moments_state = None
        if self.moments:
            from .. import denoise as D
            self.moments_state = D.moments_state(self.frame.W, self.frame.H)

    @property
    def world(self):
        return self.frame.world

    @property
    def batches(self):
        """moments=True: the batches added so far."""
        return self.samples // self.batch_spp if self.batch_spp else 0

    def features(self):
        """One-sample first-hit features of the accumulator's camera, seed and resolution (the frame's)."""
        return self.frame.features()

    def _add_batch(self, spp):
        from .. import denoise as D
        if spp == 0:
            return self
        if self.batch_spp and spp != self.batch_spp:
            raise ValueError(f"moments=True needs equal batches: add({spp}) after batches of {self.batch_spp} spp")
        batch = self.frame.add_samples(self.samples, spp)
        self.slots += batch
        D.moments_add(self.moments_state, self.frame.unpack(batch), spp, self.features(), device=self.frame.device)
        self.batch_spp = spp
        self.samples += spp
        return self

    def noise_map(self):
        """moments=True: the standard error of the demodulated luminance per pixel, (W, H) float32:
        the square root of the state's variance of the mean (0 below two batches)."""
        if not self.moments:
            raise ValueError("noise_map() needs Accumulator(..., moments=True)")
        return np.sqrt(self.moments_state[..., 3])

    def add(self, spp=1):
        """Render samples [samples, samples + spp) of every pixel onto the sums."""
        if spp < 0:
            raise ValueError("spp must be >= 0")
        if self.moments:
            return self._add_batch(int(spp))
        self.frame.add_samples(self.samples, spp, onto=self.slots)
        self.samples += spp
        return self

    def sums(self):
        """Per-pixel radiance sums (W, H, 3) [x][y] — the reference's `pixels` field."""
        return self.frame.unpack(self.slots)

    def mean(self):
        return _mean(self.sums(), self.samples)

    def denoised(self, mode="fixed", **params):
        """The running mean filtered by the a-trous denoiser (pyrenderer_amd.denoise.denoise; `params`
        are its keyword parameters), guided by one-sample first-hit features of the accumulator's own
        camera, seed and resolution: what render(..., denoise=True) returns for the same samples.
        mode="variance" routes to denoise_variance instead: render(..., denoise="variance").  With
        moments=True and at least pyrenderer_amd.denoise.MIN_MOMENT_BATCHES batches it passes the moments
        state's variance of the mean as `variance` (what render(..., variance_batches=K) does); with
        fewer batches it leaves the filter its spatial estimate."""
        from ..denoise import MIN_MOMENT_BATCHES
        if mode == "variance" and self.moments and self.batches >= MIN_MOMENT_BATCHES:
            params.setdefault("variance", self.moments_state[..., 3])   # one given by the caller wins
        return self.frame.filter(self.mean(), mode, **params)

    def state(self):
        f = self.frame
        d = dict(slots=self.slots, samples=np.int64(self.samples), seed=np.int64(f.seed), depth=np.int64(f.depth),
                 resolution=np.array([f.W, f.H], np.int64), tile=np.int64(f.tile), flags=np.int64(f.flags),
                 camera=f.cam, scene_sha=np.array(scene_fingerprint(f.world.flat)))
        if self.moments:
            d.update(moments=self.moments_state, batch_spp=np.int64(self.batch_spp))
        return d

    @staticmethod
    def state_path(path):
        """np.savez appends '.npz' to a path without it: save and load use the same name."""
        path = os.fspath(path)
        return path if path.endswith(".npz") else path + ".npz"

    def save(self, path):
        np.savez(self.state_path(path), **self.state())

    @classmethod
    def load(cls, path, scene, camera, device=0, world=None):
        z = np.load(cls.state_path(path), allow_pickle=False)
        W, H = (int(v) for v in z["resolution"])
        mis = "flags" in z.files and int(z["flags"]) & nee_flags("mis")
        acc = cls(scene, camera, depth=int(z["depth"]), seed=int(z["seed"]), resolution=(W, H), device=device,
                  tile=int(z["tile"]), world=world, nee="mis" if mis else "reference",
                  moments="moments" in z.files)
        if z["slots"].shape != acc.slots.shape:
            raise ValueError("saved accumulation does not match the frame layout")
        if "camera" in z.files and not np.array_equal(z["camera"], acc.frame.cam):
            raise ValueError("saved accumulation was rendered with a different camera")
        if "scene_sha" in z.files and str(z["scene_sha"]) != scene_fingerprint(acc.world.flat):
            raise ValueError("saved accumulation was rendered from a different scene")
        if acc.moments and z["moments"].shape != acc.moments_state.shape:
            raise ValueError("saved moments do not match the frame")
        acc.slots[...] = z["slots"]
        acc.samples = int(z["samples"])
        if acc.moments:
            acc.moments_state[...] = z["moments"]
            acc.batch_spp = int(z["batch_spp"])
        return acc


class TemporalAccumulator:
    """Rendering a camera path on one device with history carried across camera moves
    (pyrenderer_amd.denoise.temporal_accumulate; DESIGN.md §11 "Temporal accumulation").

    `add(camera)` renders frame t: samples t * spp .. t * spp + spp - 1 of every pixel from zero sums with
    that camera (one world, built at the first add), takes the frame's one-sample features, reprojects the
    previous frame's state into the new camera and blends.  `mean()` is this frame alone, `accumulated()`
    the integrated colour, `history()` the per-pixel history length (W, H), `denoised(**filter_params)` the
    integrated colour through the variance-guided filter with the state's variance plane and the spatial
    estimate where the history is short (variance_fallback="spatial").  `reset()` drops the history; the
    sample count goes on, so the next frame still draws new samples.

    `temporal_params` are temporal_accumulate's keyword parameters (alpha, alpha_m, tau_n, tau_z, tau_a,
    eps_a, min_history, w_min).  resolution: (W, H); None takes the first camera's, and every later camera
    must then have the same.  A camera with an aperture is a ValueError: a thin lens has no unique
    reprojection.  One device, no save / load.  Geometry is static unless add() is given the frame's scene:
    the history then follows rigidly moving primitives (DESIGN.md §11 "Moving objects").  Moving lights, and
    the shading changes a moving object casts on static surfaces (its shadow, its reflection), keep their
    history and lag behind by about 1 / alpha frames: SVGF's known limit.

    refit=True: a frame whose scene differs from the last one's only in its geometry updates the world this
    accumulator built in place (World.update: the trees are refit on the device, the device scene and its
    render contexts stay) instead of building a new world and closing the old one; the images are the same
    bit for bit.  A scene that differs in more, and a world the caller passed in, take the rebuild.

    rebuild_ratio (with refit=True only, else a ValueError): World.update's, a number r that has the resident
    scene's trees built again on the GPU once refits have raised tree_cost() above r times its value at the
    last build; None (default) only ever refits."""

    def __init__(self, scene, *, depth, spp, seed=0, resolution=None, device=0, tile=64, world=None, nee="reference",
                 refit=False, rebuild_ratio=None, **temporal_params):
        from .. import denoise as D
        self.refit = bool(refit)
        if rebuild_ratio is not None and not self.refit:
            raise ValueError("rebuild_ratio rebuilds the scene that refit=True keeps resident: it needs refit=True")
        if rebuild_ratio is not None and not (isinstance(rebuild_ratio, (int, float)) and rebuild_ratio > 0):
            raise ValueError(f"rebuild_ratio must be a number > 0 or None, not {rebuild_ratio!r}")
        self.rebuild_ratio = rebuild_ratio
        unknown = sorted(set(temporal_params) - set(D.TEMPORAL_PARAMS))
        if unknown:
            raise TypeError(f"unknown temporal parameter(s) {unknown}: expected some of {D.TEMPORAL_PARAMS}")
        if isinstance(spp, (bool, np.bool_)) or not isinstance(spp, (int, np.integer)) or spp < 1:
            raise ValueError(f"spp must be an integer >= 1, not {spp!r}")
        nee_flags(nee)
        self.scene, self.depth, self.spp, self.seed = scene, int(depth), int(spp), int(seed)
        self.resolution = None if resolution is None else (int(resolution[0]), int(resolution[1]))
        self._from_camera = resolution is None   # the first camera sets it, the later ones must agree
        self.device, self.tile, self.world, self.nee = device, int(tile), world, nee
        self.params = dict(temporal_params)
        self.frames = 0      # frames rendered: the next one starts at sample frames * spp
        self.frame = None    # the last frame's _Frame
        self._mean = self._color = self._state = self._prev = self._ids = None
        self._moving = False             # a scene has been passed to add(): the history follows moving objects
        self._own_world = world is None  # a world built here is released when a frame's scene replaces it

    def add(self, camera, scene=None):
        """Render the next frame with `camera` and fold it into the history.

        scene: None (default) renders the accumulator's scene; a sequence that never passes one is the static
        world of prt_temporal_accumulate.  With a scene, this frame is rendered in a world built from it, and
        from then on the history follows moving objects (prt_temporal_accumulate_motion): the motion table
        comes from the previous frame's scene (pyrenderer_amd.denoise.motion_rows: the same primitives in the
        same order, e.g. pyrenderer_amd.scenes.moved), the object-id planes of both frames are kept, and the
        previous frame's device scene is released.  Passing the scene the last frame used builds nothing."""
        from .. import denoise as D
        if camera.aperture > 0:
            raise ValueError("TemporalAccumulator needs a pinhole camera: a thin lens (aperture > 0) has no unique "
                             "reprojection")
        res = tuple(int(v) for v in camera.resolution)
        if self.resolution is None:
            self.resolution = res
        elif self._from_camera and res != self.resolution:
            raise ValueError(f"the resolution cannot change within a sequence: {res} after {self.resolution}")
        motion = None
        if scene is not None or self._moving:
            scene = self.scene if scene is None else scene
            # raises before anything is built or rendered
            motion = D.motion_rows(scene if self.scene is None else self.scene, scene)
        if self._prev is not None and motion is not None:
            # the last frame's id plane, due now after a static frame: composed while the device scene still
            # holds that frame's pose (a refit below moves it in place)
            self.object_ids()
        stale = None
        if scene is not None and scene is not self.scene:
            if not self._refit_world(scene):
                stale, self.world, self._own_world = (self.world if self._own_world else None), None, True
            self.scene = scene
        if self.world is None:
            self.world = build_world(self.scene, (self.device,))
            self._own_world = True
        f = _Frame.of(self.scene, camera, depth=self.depth, seed=self.seed, resolution=self.resolution,
                      devices=(self.device,), tile=self.tile, world=self.world, nee=self.nee)
        mean = _mean(f.unpack(f.add_samples(self.frames * self.spp, self.spp)), self.spp)
        feat = f.features()
        moving = motion is not None
        ids = D.object_ids(f.ds, f.cam, f.W, f.H) if moving else None
        prev = self._prev
        if prev is not None and moving:   # the last frame's plane: kept, or due now after a static frame
            prev = (*prev, self.object_ids())
        state, color = D.temporal_accumulate(mean, feat, f.cam, prev, device=self.device, ids=ids, motion=motion,
                                             **self.params)
        self._moving, self._prev, self._ids = moving, (state, feat, f.cam), ids
        self.frame, self._mean, self._color, self._state = f, mean, color, state
        if stale is not None:   # the previous frame's world: nothing reads it any more
            for ds in stale.device_scenes.values():
                ds.close()
        self.frames += 1
        return self

    def _refit_world(self, scene):
        """refit=True and a world of this accumulator's own: update it in place to `scene`; False when that is
        not possible (the caller then rebuilds)."""
        if not (self.refit and self._own_world and self.world is not None):
            return False
        try:
            self.world.update(scene.primitives, rebuild_ratio=self.rebuild_ratio)
        except ValueError:   # more than the geometry differs
            return False
        return True

    def object_ids(self):
        """The last frame's object-id plane, (W, H) int32 (pyrenderer_amd.denoise.object_ids): the plane the
        accumulation used, or for a static sequence one composed on demand."""
        self._need_frame()
        if self._ids is None:
            from .. import denoise as D
            self._ids = D.object_ids(self.frame.ds, self.frame.cam, self.frame.W, self.frame.H)
        return self._ids

    def _need_frame(self):
        if self.frame is None:
            raise ValueError("no frame yet: add(camera) first")

    def mean(self):
        """This frame's Monte-Carlo mean alone, (W, H, 3)."""
        self._need_frame()
        return self._mean

    def accumulated(self):
        """The integrated colour, re-modulated, (W, H, 3)."""
        self._need_frame()
        return self._color

    def history(self):
        """The history length per pixel, (W, H) float32: 1 where this frame started afresh, 0 at a pixel that
        is not finite."""
        self._need_frame()
        return self._state[..., 3]

    def state(self):
        """The temporal state, (W, H, 8) float32: I.rgb, h, m1, m2, the variance plane, 0."""
        self._need_frame()
        return self._state

    def features(self):
        """This frame's one-sample first-hit features."""
        self._need_frame()
        return self.frame.features()

    def denoised(self, **filter_params):
        """accumulated() through denoise_variance with the temporal variance and the spatial fallback."""
        self._need_frame()
        filter_params.setdefault("variance", self._state[..., 6])
        filter_params.setdefault("variance_fallback", "spatial")
        return self.frame.filter(self._color, "variance", **filter_params)

    def reset(self):
        """Forget the history: the next frame starts afresh at every pixel."""
        self._prev = None
        return self


def render_sequence(scene, cameras, *, spp, depth, seed=0, resolution=None, device=0, tile=64, world=None,
                    nee="reference", denoise="variance", scenes=None, refit=False, rebuild_ratio=None,
                    **temporal_params):
    """The frames of a camera path with temporal accumulation, (n, W, H, 3) float32: frame t is
    TemporalAccumulator.add(cameras[t]) followed by denoised() (denoise="variance", the default) or
    accumulated() (denoise=False).  Anything else is a ValueError.  scenes: None (default) is the static
    `scene`; one scene per camera makes frame t add(cameras[t], scenes[t]), the history following the
    primitives that move between them; refit=True then refits the resident scene between frames instead of
    rebuilding it (TemporalAccumulator's refit), same images, and rebuild_ratio= (with refit=True only) has its
    trees built again on the GPU once the refits have loosened them that far (TemporalAccumulator's)."""
    if not ((isinstance(denoise, str) and denoise == "variance") or denoise is False):
        raise ValueError(f"denoise must be 'variance' or False, not {denoise!r}")
    cameras = list(cameras)
    if not cameras:
        raise ValueError("render_sequence needs at least one camera")
    if scenes is not None:
        scenes = list(scenes)
        if len(scenes) != len(cameras):
            raise ValueError(f"scenes must hold one scene per camera: {len(scenes)} for {len(cameras)} cameras")
    acc = TemporalAccumulator(scene, depth=depth, spp=spp, seed=seed, resolution=resolution, device=device, tile=tile,
                              world=world, nee=nee, refit=refit, rebuild_ratio=rebuild_ratio, **temporal_params)
    out = []
    for t, cam in enumerate(cameras):
        acc.add(cam, None if scenes is None else scenes[t])
        out.append(acc.denoised() if denoise else acc.accumulated())
    return np.stack(out).astype(np.float32)


def render_adaptive(scene, camera, *, depth, batch_spp, max_batches, target, min_batches=2, tolerate=0.0, eps_r=None,
                    seed=0, resolution=None, device=0, tile=64, world=None, nee="reference", denoise=False,
                    return_samples=False):
    """Mean linear radiance (W, H, 3) float32 rendered in batches of batch_spp samples, at most max_batches of
    them per tile, that stops every tile once its noise has reached `target`
    (pyrenderer_amd.adaptive.AdaptiveAccumulator, whose parameters these are): run(max_batches)
    followed by mean(), or by denoised() for denoise=True (the fixed filter) or "variance".  With
    return_samples=True the pair (image, (W, H) int32 samples per pixel).  One device; render() and its
    defaults are untouched by it."""
    if not (isinstance(denoise, (bool, np.bool_)) or (isinstance(denoise, str) and denoise == "variance")):
        raise ValueError(f"denoise must be False, True or 'variance', not {denoise!r}")
    if isinstance(max_batches, (bool, np.bool_)) or not isinstance(max_batches, (int, np.integer)) or max_batches < 1:
        raise ValueError(f"max_batches must be an integer >= 1, not {max_batches!r}")
    from .. import adaptive as A   # imports torch: only this entry point pays for it
    kw = {} if eps_r is None else dict(eps_r=eps_r)
    acc = A.AdaptiveAccumulator(scene, camera, depth=depth, batch_spp=batch_spp, target=target,
                                min_batches=min_batches, tolerate=tolerate, seed=seed, resolution=resolution,
                                device=device, tile=tile, world=world, nee=nee, **kw)
    acc.run(int(max_batches))
    if not denoise:
        img = acc.mean()
    else:
        img = acc.denoised("variance" if isinstance(denoise, str) else "fixed")
    return (img, acc.samples()) if return_samples else img


def scene_fingerprint(flat):
    """SHA-256 (hex, 16 chars) of the flattened scene arrays the kernel renders."""
    h = hashlib.sha256()
    for k in ("tri_v", "tri_n", "tri_mat", "mat", "light_tri", "light_off", "direct_rgb", "sph", "sph_mat"):
        a = getattr(flat, k, None)
        if a is not None:
            a = np.ascontiguousarray(a)
            h.update(k.encode() + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()[:16]


def as_image(radiance_xy):
    """[x][y] (y up) → [row][col] top row first, as main.py:55 writes images."""
    return np.ascontiguousarray(np.asarray(radiance_xy).transpose(1, 0, 2)[::-1])

"""Adaptive sampling: render in batches and stop the tiles whose noise has reached a target.

Random streams are keyed by (seed, pixel, sample) and every render call takes a tile list, so batch b of a
subset of tiles holds, for those tiles, exactly the bits a full-frame render of batch b would.
`AdaptiveAccumulator` renders batch after batch of the tiles that are still active, folds each into the frame's
radiance sums and per-pixel moments on the device (prt_adaptive_update_device, one fused HIP kernel that
also scores every tile) and stops a tile once no more than a tolerated share of its pixels is over the target:
a tile that ran k batches holds what Accumulator(moments=True) holds there after k equal add()s, bit for bit.

The policy, `still_active`, is a pure NumPy function of the kernel's tile records.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .denoise import EPS_A, MIN_MOMENT_BATCHES

EPS_R = 1e-3          # floor of the relative error's denominator, in demodulated luminance
RECORD_WORDS = 4      # pixels in the frame, pixels over the target, bits of the greatest error, young pixels


def check_policy(min_batches, tolerate):
    """The policy's parameters: min_batches an integer >= 2 (one batch has no variance), tolerate in [0, 1)."""
    if isinstance(min_batches, (bool, np.bool_)) or not isinstance(min_batches, (int, np.integer)) or min_batches < 2:
        raise ValueError(f"min_batches must be an integer >= 2, not {min_batches!r}")
    if isinstance(tolerate, (bool, np.bool_)) or not (0.0 <= float(tolerate) < 1.0):
        raise ValueError(f"tolerate must be in [0, 1), not {tolerate!r}")
    return int(min_batches), float(tolerate)


def still_active(records, b, min_batches=2, tolerate=0.0):
    """Which of the tiles with the records `records` ((n, 4) uint32, prt_adaptive_update's) go on after their
    b-th batch: (n,) bool.  A tile stops when b >= min_batches and the pixels over the target, records[:, 1],
    are at most floor(tolerate * records[:, 0]), its pixels inside the frame."""
    min_batches, tolerate = check_policy(min_batches, tolerate)
    rec = np.asarray(records)
    if rec.ndim != 2 or rec.shape[1] != RECORD_WORDS:
        raise ValueError(f"records must be (n, {RECORD_WORDS}), not {rec.shape}")
    if int(b) < min_batches:
        return np.ones(rec.shape[0], bool)
    allowed = np.floor(tolerate * rec[:, 0].astype(np.float64)).astype(np.int64)
    return rec[:, 1].astype(np.int64) > allowed


def check_sampler(batch_spp, target, min_batches, tolerate, eps_r):
    """AdaptiveAccumulator's own parameters, before any scene or device is touched."""
    if isinstance(batch_spp, (bool, np.bool_)) or not isinstance(batch_spp, (int, np.integer)) or batch_spp < 1:
        raise ValueError(f"batch_spp must be an integer >= 1, not {batch_spp!r}")
    if isinstance(target, (bool, np.bool_)) or not (float(target) >= 0.0):
        raise ValueError(f"target must be >= 0 (inf is allowed), not {target!r}")
    if not (float(eps_r) > 0.0 and np.isfinite(eps_r)):
        raise ValueError(f"eps_r must be positive and finite, not {eps_r!r}")
    return check_policy(min_batches, tolerate)


def _vp(address):
    return ctypes.c_void_p(address) if address else None


def adaptive_update_device(d_batch_ptr, tile_ids, tw, th, W, H, d_feat_ptr, n_samples, d_sum_ptr, d_state_ptr,
                           d_records_ptr, *, target, eps_r=EPS_R, eps_a=EPS_A, device=0, stream_ptr=None):
    """prt_adaptive_update_device: one batch of the tiles `tile_ids` (host ids; the batch's slots on the device at
    d_batch_ptr) folded into the device planes d_sum_ptr (W x H x 3) and d_state_ptr (W x H x 4, 16-byte
    aligned), the tiles' records into d_records_ptr (n_tiles x 4 u32); enqueued on `stream_ptr` without a host
    synchronisation."""
    ids = np.ascontiguousarray(tile_ids, np.int32)
    par = np.array([eps_r, target], np.float32)
    N.check_denoise(N.lib().prt_adaptive_update_device(
        int(device), _vp(d_batch_ptr), N.ptr(ids), ids.shape[0], int(tw), int(th), int(W), int(H), _vp(d_feat_ptr),
        float(eps_a), float(n_samples), N.ptr(par), _vp(d_sum_ptr), _vp(d_state_ptr), _vp(d_records_ptr),
        _vp(stream_ptr)))


def adaptive_update(io_sum, io_state, batch, tile_ids, tw, th, feat, n_samples, *, target, eps_r=EPS_R, eps_a=EPS_A,
                    device=0):
    """prt_adaptive_update on host arrays: io_sum (W, H, 3) and io_state (W, H, 4) are updated in place; returns
    the records (n_tiles, 4) uint32 in the order of tile_ids."""
    for name, a, c in (("io_sum", io_sum, 3), ("io_state", io_state, 4)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.ndim == 3
                and a.shape[2] == c):
            raise ValueError(f"{name} must be a C-contiguous float32 (W, H, {c}) array")
    W, H = io_sum.shape[:2]
    if io_state.shape[:2] != (W, H):
        raise ValueError(f"io_state must be {(W, H, 4)}, not {io_state.shape}")
    ids = np.ascontiguousarray(tile_ids, np.int32).reshape(-1)
    batch = np.ascontiguousarray(batch, np.float32)
    if batch.size != ids.shape[0] * int(tw) * int(th) * 3:
        raise ValueError(f"batch must hold {ids.shape[0]} x {tw} x {th} x 3 floats, not {batch.size}")
    feat = np.ascontiguousarray(feat, np.float32)
    if feat.shape != (W, H, 8):
        raise ValueError(f"feat must be {(W, H, 8)}, not {feat.shape}")
    records = np.zeros((ids.shape[0], RECORD_WORDS), np.uint32)
    par = np.array([eps_r, target], np.float32)
    N.check_denoise(N.lib().prt_adaptive_update(int(device), N.ptr(batch), N.ptr(ids), ids.shape[0], int(tw), int(th),
                                                W, H, N.ptr(feat), float(eps_a), float(n_samples), N.ptr(par),
                                                N.ptr(io_sum), N.ptr(io_state), N.ptr(records)))
    return records


class AdaptiveAccumulator:
    """Progressive rendering on one device that stops converged tiles.

    `step()` renders the next batch of `batch_spp` samples of the tiles that are still active (all of them share
    the batch index: a tile that has stopped never resumes), folds it in and applies the policy; it returns how
    many tiles remain active.  `run(max_batches)` steps until none does or `max_batches` batches are done.

    target: the relative standard error of the demodulated luminance, sqrt(var_mean) / (|mean| + eps_r), a
    pixel must not exceed.  A tile stops after its b-th batch when b >= min_batches and at most
    floor(tolerate * its pixels) pixels are over the target; a pixel with fewer than two batches counts as over.

    Features, sums, moments state and records live in torch tensors on the device.  Each round copies the
    rendered batch from the host to the device (the render call that leaves a batch with a first sample on
    the device does not exist yet) and reads the records back: the one synchronisation per round."""

    def __init__(self, scene, camera, *, depth, batch_spp, target, min_batches=2, tolerate=0.0, eps_r=EPS_R, seed=0,
                 resolution=None, device=0, tile=64, world=None, nee="reference"):
        self.min_batches, self.tolerate = check_sampler(batch_spp, target, min_batches, tolerate, eps_r)
        from .core.tracing import _Frame
        self.batch_spp, self.target, self.eps_r = int(batch_spp), float(target), float(eps_r)
        self.frame = f = _Frame.of(scene, camera, depth=depth, seed=seed, resolution=resolution, devices=(device,),
                                   tile=tile, world=world, nee=nee)
        self.dev = torch.device("cuda", f.device)
        W, H = f.W, f.H
        n = f.ids.shape[0]
        self.d_feat = torch.zeros((W, H, 8), dtype=torch.float32, device=self.dev)
        self.d_sum = torch.zeros((W, H, 3), dtype=torch.float32, device=self.dev)
        self.d_state = torch.zeros((W, H, 4), dtype=torch.float32, device=self.dev)
        self.d_records = torch.zeros((n, RECORD_WORDS), dtype=torch.int32, device=self.dev)
        stream = torch.cuda.current_stream(self.dev)
        # the features _Frame.features() gives: one sample, first sample 0, the frame's seed
        f.ds.features_device(f.cam, W, H, self.d_feat.data_ptr(), samples=1, first_sample=0, seed=f.seed,
                             stream_ptr=stream.cuda_stream)
        self.batches = 0                                    # batches rendered: the active tiles' shared index
        self.active = np.ones(n, bool)                      # by tile id
        self.batches_per_tile = np.zeros(n, np.int32)       # by tile id
        self._records = np.zeros((n, RECORD_WORDS), np.uint32)

    @property
    def world(self):
        return self.frame.world

    def step(self):
        """One round: the next batch of the active tiles.  Returns the number of tiles still active."""
        f = self.frame
        ids = np.nonzero(self.active)[0].astype(np.int32)
        if ids.shape[0] == 0:
            return 0
        batch = f.add_samples(self.batches * self.batch_spp, self.batch_spp, ids=ids)
        stream = torch.cuda.current_stream(self.dev)
        d_batch = torch.from_numpy(batch).to(self.dev)
        d_rec = self.d_records[:ids.shape[0]]
        adaptive_update_device(d_batch.data_ptr(), ids, f.tile, f.tile, f.W, f.H, self.d_feat.data_ptr(),
                               self.batch_spp, self.d_sum.data_ptr(), self.d_state.data_ptr(), d_rec.data_ptr(),
                               target=self.target, eps_r=self.eps_r, device=f.device, stream_ptr=stream.cuda_stream)
        rec = d_rec.cpu().numpy().view(np.uint32)   # the round's one synchronisation
        self.batches += 1
        self.batches_per_tile[ids] = self.batches
        self._records[ids] = rec
        self.active[ids] = still_active(rec, self.batches, self.min_batches, self.tolerate)
        return int(self.active.sum())

    def run(self, max_batches):
        """step() until no tile is active or `max_batches` batches have been rendered; returns self."""
        if isinstance(max_batches, (bool, np.bool_)) or not isinstance(max_batches, (int, np.integer)) or max_batches < 0:
            raise ValueError(f"max_batches must be an integer >= 0, not {max_batches!r}")
        while self.batches < max_batches and self.active.any():
            self.step()
        return self

    def _per_pixel(self, per_tile):
        f = self.frame
        tiles_x = (f.W + f.tile - 1) // f.tile
        tx, ty = np.arange(f.W) // f.tile, np.arange(f.H) // f.tile
        return per_tile[ty[None, :] * tiles_x + tx[:, None]]

    def samples(self):
        """Samples per pixel, (W, H) int32: the pixel's tile's batches times batch_spp."""
        return (self._per_pixel(self.batches_per_tile) * np.int32(self.batch_spp)).astype(np.int32)

    def sums(self):
        """Per-pixel radiance sums (W, H, 3) [x][y]."""
        return self.d_sum.cpu().numpy()

    def mean(self):
        """sums / samples, one float32 division; zeros where no sample was taken."""
        n = self.samples().astype(np.float32)[..., None]
        sums = self.sums()
        return np.where(n > 0, sums / np.where(n > 0, n, np.float32(1.0)), np.float32(0.0)).astype(np.float32)

    def moments(self):
        """The moments state (W, H, 4): k, mean, M2, var_mean (pyrenderer_amd.denoise.moments_add's)."""
        return self.d_state.cpu().numpy()

    def noise_map(self):
        """The standard error of the demodulated luminance per pixel, (W, H) float32."""
        return np.sqrt(self.moments()[..., 3])

    def records(self):
        """Every tile's last record, (n_tiles, 4) uint32 by tile id."""
        return self._records.copy()

    def features(self):
        """The one-sample first-hit features of the frame, (W, H, 8)."""
        if self.frame._feat is None:
            self.frame._feat = self.d_feat.cpu().numpy()
        return self.frame._feat

    def spent(self, max_batches):
        """The share of max_batches batches of every tile that was actually rendered, by pixels."""
        if max_batches <= 0:
            return 0.0
        s = self.samples().astype(np.float64)
        return float(s.sum() / (s.size * float(max_batches) * self.batch_spp))

    def denoised(self, mode="fixed", **params):
        """mean() through the a-trous filter, guided by features().  mode="variance" passes the moments
        state's variance of the mean as `variance` once every tile holds
        pyrenderer_amd.denoise.MIN_MOMENT_BATCHES batches, as Accumulator does; below that the filter keeps its
        spatial estimate."""
        self.features()
        if mode == "variance" and int(self.batches_per_tile.min()) >= MIN_MOMENT_BATCHES:
            params.setdefault("variance", self.moments()[..., 3])
        return self.frame.filter(self.mean(), mode, **params)

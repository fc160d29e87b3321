"""The inputs of the sample-moments tests on the GPU (tests/test_gpu_moments.py, tests/test_gpu_adaptive.py):
the filter parameters, the finiteness bound and the frames with their features.  Pure NumPy."""
import numpy as np

F32 = np.float32
PAR = dict(sigma_l=1.5, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3, eps_l=3e-3)
N_SAMPLES = 4.0
BOUND = 2.0 ** 62   # include/prt.h: |l| <= 2^62 keeps the state finite for up to 8 frames


def features(W, H, rng):
    """Albedos in [0.02, 1], a depth ramp, mostly one normal; a block of miss pixels as features() writes
    them and (from 4 pixels on) albedos below eps_a with one channel exactly 0."""
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = rng.uniform(0.02, 1.0, (W, H, 3))
    n = rng.normal(size=(W, H, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    F[..., 3:6] = np.where(rng.uniform(size=(W, H, 1)) < 0.7, np.array([0.0, 0.6, 0.8]), n)
    F[..., 6] = 1.5 + 0.03 * np.arange(W)[:, None] + 0.011 * np.arange(H)[None, :] + rng.uniform(0, 0.01, (W, H))
    F[..., 7] = rng.choice([0.25, 0.5, 1.0], (W, H))
    if W * H >= 4:
        idx = rng.permutation(W * H)[: max(1, W * H // 10)]
        for k in idx:
            F[k // H, k % H, 0:3] = (1e-3, 0.0, 5e-3)
        x0, y0 = W // 3, H // 4
        F[x0:x0 + max(1, W // 4), y0:y0 + max(1, H // 3)] = 0.0
    return F


def frames(W, H, K, seed):
    """K frames of radiance sums over N_SAMPLES samples and their features; the last pixel holds the
    finiteness bound with alternating sign (albedo 1) and, from 4 pixels on, one pixel a NaN in frame 0
    and one a +inf in the last frame."""
    rng = np.random.default_rng(seed)
    F = features(W, H, rng)
    S = (N_SAMPLES * np.fmax(F[None, ..., 0:3], 0.05) * rng.uniform(0.3, 1.7, (K, W, H, 3))).astype(F32)
    F[W - 1, H - 1] = (1.0, 1.0, 1.0, 0.0, 0.0, 1.0, 2.0, 1.0)
    S[:, W - 1, H - 1] = (np.where(np.arange(K) % 2 == 0, 1.0, -1.0) * BOUND * N_SAMPLES)[:, None]
    if W * H >= 4:
        hits = np.argwhere(F[..., 7] > 0)
        (ax, ay), (bx, by) = hits[len(hits) // 3], hits[len(hits) // 2]
        S[0, ax, ay, 1] = np.nan
        S[K - 1, bx, by, 2] = np.inf
    return S, F

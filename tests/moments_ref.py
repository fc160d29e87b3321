"""NumPy float32 restatement of the sample-moments kernels (pyrenderer_amd/csrc/prt_denoise.hip:
moments_kernel and var_given_kernel).

A helper module like atrous_ref.py and atrous_var_ref.py.  `moments_add(state, frames, n, feat, eps_a)`
returns what prt_moments_add leaves in the state and `atrous_var_given(color, feat, in_var, ...)` what
prt_denoise_var_given returns, bit for bit.

moments, per pixel, state (k, mean, M2, var_mean), for each frame of radiance sums S in order
    c_c  = S_c / n
    I_c  = c_c / fmax(A_c, eps_a) if F[7] > 0 else c_c
    l    = (0.2126 * I_r + 0.7152 * I_g) + 0.0722 * I_b
    a frame whose l is not finite leaves the pixel's state as it is
    k'   = k + 1;  d = l - mean;  mean' = mean + d / k';  M2' = M2 + d * (l - mean')
after the last frame
    var_mean = (M2 / (k - 1)) / k if k >= 2 else 0;  a var_mean that is not finite becomes 0

given variance: atrous_var_ref.atrous_var with its `estimate` replaced by
    v = in_var if the pixel is usable (hit and not bad) and in_var is finite and >= 0, else 0
(-0 >= 0 holds, so a -0 is passed on as -0).
"""
import numpy as np

import atrous_ref as R
import atrous_var_ref as V

F32 = np.float32


def moments_add(state, frames, n, feat, eps_a=1e-2):
    """The state after adding `frames` ((n_frames, W, H, 3) sums of n samples each): a new (W, H, 4) array."""
    S = np.ascontiguousarray(frames, F32)
    if S.ndim == 3:
        S = S[None]
    F = np.ascontiguousarray(feat, F32)
    st = np.array(state, F32, copy=True)
    n, eps_a = F32(n), F32(eps_a)
    hit = F[..., 7] > 0
    a = np.fmax(F[..., 0:3], eps_a)
    k, mean, m2 = st[..., 0].copy(), st[..., 1].copy(), st[..., 2].copy()
    with np.errstate(all="ignore"):
        for f in range(S.shape[0]):
            c = (S[f] / n).astype(F32)
            I = np.where(hit[..., None], c / a, c).astype(F32)
            l = V.lum(I).astype(F32)
            ok = np.isfinite(l)
            k1 = k + F32(1.0)
            d = l - mean
            mean1 = mean + d / k1
            m21 = m2 + d * (l - mean1)
            k = np.where(ok, k1, k).astype(F32)
            mean = np.where(ok, mean1, mean).astype(F32)
            m2 = np.where(ok, m21, m2).astype(F32)
        vm = (m2 / np.where(k >= 2, k - F32(1.0), F32(1.0))) / np.where(k >= 2, k, F32(1.0))
        vm = np.where(k >= 2, vm, F32(0.0))
        vm = np.where(np.isfinite(vm), vm, F32(0.0))
    return np.stack([k, mean, m2, vm.astype(F32)], axis=-1).astype(F32)


def given(in_var, live):
    """var_given_kernel's variance plane."""
    t = np.ascontiguousarray(in_var, F32)
    with np.errstate(all="ignore"):
        return np.where(live & np.isfinite(t) & (t >= 0), t, F32(0.0)).astype(F32)


def atrous_var_given(color, feat, in_var, iterations=5, sigma_l=1.0, sigma_z=2.0, eps_a=1e-2, eps_z=1e-2, eps_l=1e-2):
    """prt_denoise_var_given: ((W, H, 3) image, (W, H) variance actually used), both float32."""
    C = np.ascontiguousarray(color, F32)
    I, Z, N, gx, gy, hit, bad, a = R.prepass(C, feat, eps_a)
    live = hit & ~bad
    used = given(in_var, live)
    Vp = used
    for i in range(int(iterations)):
        I, Vp = V.one_pass(I, Vp, Z, N, gx, gy, live, 1 << i, sigma_l, sigma_z, eps_z, eps_l)
    with np.errstate(all="ignore"):
        out = np.where(hit[..., None], I * a, I)
    out = np.where(bad[..., None], C, out).astype(F32)
    return out, used

"""NumPy float32 restatement of the variance-guided a-trous mode (prt_denoise_var,
pyrenderer_amd/csrc/prt_denoise.hip: var_estimate_kernel and pass_kernel<true>).

A helper module like atrous_ref.py, whose pre-pass, post-pass, e(x) and tap windows it shares.
`atrous_var(color, feat, iterations, sigma_l, sigma_z, eps_a, eps_z, eps_l)` returns what
prt_denoise_var returns, bit for bit: the filtered image and the variance estimate.

"Usable tap": inside the frame, hit and not bad, seen from a centre that is hit and not bad.

luminance
    l(I) = (0.2126 * I_r + 0.7152 * I_g) + 0.0722 * I_b

variance estimate, per usable pixel p (every other pixel: var = 0)
    for dx = -3 .. 3 (outer), dy = -3 .. 3 (inner), q = p + (dx, dy) usable:
        centre: w = 1
        others: w = wn * e(xz) with atrous_ref's wn and xz at step 1
        sw = sw + w;  m1 = m1 + w * l_q;  m2 = m2 + w * (l_q * l_q)
    mu = m1 / sw;  var = fmax(0, m2 / sw - mu * mu);  a var that is not finite becomes 0

pass i = 0 .. n-1, step s = 2^i, per usable pixel p (every other pixel keeps colour and variance)
    for dx = -1 .. 1 (outer), dy = -1 .. 1 (inner), q = p + (dx, dy) usable (never step-scaled):
        g = (1/4, 1/8, 1/16)[|dx| + |dy|];  gv = gv + g * var_q;  gs = gs + g
    sd = sqrt(gv / gs);  den = sigma_l * sd + eps_l
    the 25 taps of atrous_ref's pass, with
        xl = |l(I_p) - l(I_q)| / den
        w  = ((h * wn) * e(xz)) * e(xl),  centre tap w = h
        sum_w = sum_w + w;  sum_c = sum_c + w * I_q,c;  sum_v = sum_v + (w * w) * var_q
    I'_c = sum_c / sum_w;  var' = sum_v / (sum_w * sum_w);  a var' that is not finite becomes 0
"""
import numpy as np

import atrous_ref as R

F32 = np.float32
G = (F32(0.25), F32(0.125), F32(0.0625))


def lum(I):
    return (F32(0.2126) * I[..., 0] + F32(0.7152) * I[..., 1]) + F32(0.0722) * I[..., 2]


def _normal_weight(Np, Nq):
    wn = np.fmax(F32(0.0), (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2])
    for _ in range(7):
        wn = wn * wn
    return wn


def _xz(Z, gx, gy, p, q, ox, oy, sigma_z, eps_z):
    gd = gx[p] * F32(ox) + gy[p] * F32(oy)
    return np.abs(Z[p] - Z[q]) / (sigma_z * np.abs(gd) + eps_z)


def estimate(I, Z, N, gx, gy, live, sigma_z, eps_z):
    """The variance estimate of the demodulated luminance, (W, H) float32."""
    W, H = Z.shape
    sigma_z, eps_z = F32(sigma_z), F32(eps_z)
    L = lum(I).astype(F32)
    sw = np.zeros((W, H), F32)
    m1 = np.zeros((W, H), F32)
    m2 = np.zeros((W, H), F32)
    with np.errstate(all="ignore"):
        for dx in range(-3, 4):
            for dy in range(-3, 4):
                win = R._window(W, H, dx, dy)
                if win is None:
                    continue
                p, q = win
                take = live[p] & live[q]
                if dx == 0 and dy == 0:
                    w = np.ones(take.shape, F32)
                else:
                    w = _normal_weight(N[p], N[q]) * R.e16(_xz(Z, gx, gy, p, q, dx, dy, sigma_z, eps_z))
                lq = L[q]
                sw[p] = np.where(take, sw[p] + w, sw[p])
                m1[p] = np.where(take, m1[p] + w * lq, m1[p])
                m2[p] = np.where(take, m2[p] + w * (lq * lq), m2[p])
        safe = np.where(live, sw, F32(1.0))
        mu = m1 / safe
        var = np.fmax(F32(0.0), m2 / safe - mu * mu)
        var = np.where(np.isfinite(var), var, F32(0.0))
    return np.where(live, var, F32(0.0)).astype(F32)


def one_pass(I, V, Z, N, gx, gy, live, step, sigma_l, sigma_z, eps_z, eps_l):
    """One variance-guided pass: (I', var')."""
    W, H = Z.shape
    sigma_l, sigma_z, eps_z, eps_l = F32(sigma_l), F32(sigma_z), F32(eps_z), F32(eps_l)
    with np.errstate(all="ignore"):
        gv = np.zeros((W, H), F32)
        gs = np.zeros((W, H), F32)
        for dx in range(-1, 2):
            for dy in range(-1, 2):
                win = R._window(W, H, dx, dy)
                if win is None:
                    continue
                p, q = win
                take = live[p] & live[q]
                g = G[abs(dx) + abs(dy)]
                gv[p] = np.where(take, gv[p] + g * V[q], gv[p])
                gs[p] = np.where(take, gs[p] + g, gs[p])
        sd = np.sqrt(gv / np.where(live, gs, F32(1.0)))
        den = (sigma_l * sd + eps_l).astype(F32)
        L = lum(I).astype(F32)
        sum_w = np.zeros((W, H), F32)
        acc = np.zeros((W, H, 3), F32)
        sum_v = np.zeros((W, H), F32)
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                win = R._window(W, H, step * dx, step * dy)
                if win is None:
                    continue
                p, q = win
                take = live[p] & live[q]
                h = R.K[abs(dx)] * R.K[abs(dy)]
                Iq = I[q]
                if dx == 0 and dy == 0:
                    w = np.full(take.shape, h, F32)
                else:
                    xz = _xz(Z, gx, gy, p, q, step * dx, step * dy, sigma_z, eps_z)
                    xl = np.abs(L[p] - L[q]) / den[p]
                    w = ((h * _normal_weight(N[p], N[q])) * R.e16(xz)) * R.e16(xl)
                sum_w[p] = np.where(take, sum_w[p] + w, sum_w[p])
                acc[p] = np.where(take[..., None], acc[p] + w[..., None] * Iq, acc[p])
                sum_v[p] = np.where(take, sum_v[p] + (w * w) * V[q], sum_v[p])
        safe = np.where(live, sum_w, F32(1.0))
        out = np.where(live[..., None], acc / safe[..., None], I)
        var = sum_v / (safe * safe)
        var = np.where(np.isfinite(var), var, F32(0.0))
        var = np.where(live, var, V)
    return out.astype(F32), var.astype(F32)


def atrous_var(color, feat, iterations=5, sigma_l=1.0, sigma_z=2.0, eps_a=1e-2, eps_z=1e-2, eps_l=1e-2,
               return_final_variance=False):
    """prt_denoise_var on (W, H, 3) colour and (W, H, 8) features: ((W, H, 3) image, (W, H) variance
    estimate), both float32; with return_final_variance also the variance carried out of the last pass."""
    C = np.ascontiguousarray(color, F32)
    I, Z, N, gx, gy, hit, bad, a = R.prepass(C, feat, eps_a)
    live = hit & ~bad
    est = estimate(I, Z, N, gx, gy, live, sigma_z, eps_z)
    V = est
    for i in range(int(iterations)):
        I, V = one_pass(I, V, Z, N, gx, gy, live, 1 << i, sigma_l, sigma_z, eps_z, eps_l)
    with np.errstate(all="ignore"):
        out = np.where(hit[..., None], I * a, I)
    out = np.where(bad[..., None], C, out).astype(F32)
    return (out, est, V) if return_final_variance else (out, est)

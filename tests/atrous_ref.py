"""NumPy float32 restatement of the a-trous denoiser (pyrenderer_amd/csrc/prt_denoise.hip).

A helper module for the denoiser's tests, not a conftest.  `atrous(color, feat, iterations,
sigma_c, sigma_z, eps_a, eps_z)` computes what prt_denoise computes, bit for bit: every value is
a float32 array, every operation one IEEE f32 add, mul, div, sqrt, min, max or abs, vectorised
per tap over shifted arrays with the kernel's accumulation order.

Association (the kernel's; both sides follow it):

pre-pass, per pixel p of the [x][y] frames
    hit   = F[7] > 0
    a_c   = fmax(F[c], eps_a)                       c = 0, 1, 2   (fmax: a NaN albedo gives eps_a)
    I_c   = C_c / a_c if hit else C_c
    bad   = any C_c, I_c or F[0..7] not finite      (a finite colour may overflow over a tiny albedo;
                                                     a non-finite feature would make weights NaN)
    len   = sqrt((nx*nx + ny*ny) + nz*nz);  N^ = N / len per component if len > 0 else 0
    gx    = 0.5 * (Z[min(x+1, W-1)][y] - Z[max(x-1, 0)][y]),  gy likewise along y;
            a gx or gy that is not finite (a neighbour's depth is not) is replaced by 0

pass i = 0 .. n-1, step s = 2^i, sc2 = sc * sc with sc = sigma_c * (1 / 2^i)
    a pixel that is bad or not hit keeps its value (a miss has no surface: N^ = 0 gives every
    tap but its own weight 0, and keeping the value avoids the rounding of (h * I) / h)
    for dx = -2 .. 2 (outer), dy = -2 .. 2 (inner), q = p + s * (dx, dy):
        skipped when q is outside the frame, bad_q, or not hit_q
        h  = k[|dx|] * k[|dy|],  k = (3/8, 1/4, 1/16)
        centre tap: w = h
        others:     wn = fmax(0, (nx*nx' + ny*ny') + nz*nz'), squared seven times
                    gd = gx * float(s*dx) + gy * float(s*dy)
                    xz = |Z_p - Z_q| / (sigma_z * |gd| + eps_z)
                    xc = ((dr*dr + dg*dg) + db*db) / sc2,   d = I_p - I_q
                    e(x): r = 1 / (1 + x * 0.0625), squared four times
                    w  = ((h * wn) * e(xz)) * e(xc)
        sum_w = sum_w + w;  sum_c = sum_c + w * I_q,c
    I'_c = sum_c / sum_w

post-pass
    out_c = C_c if bad, I_c * fmax(F[c], eps_a) if hit, else I_c
"""
import numpy as np

F32 = np.float32
K = (F32(0.375), F32(0.25), F32(0.0625))


def e16(x):
    """e(x) = (1 / (1 + x / 16))^16 by four squarings (x / 16 == x * 0.0625 exactly)."""
    x = np.asarray(x, F32)
    r = F32(1.0) / (F32(1.0) + x * F32(0.0625))
    for _ in range(4):
        r = r * r
    return r


def prepass(color, feat, eps_a):
    C = np.ascontiguousarray(color, F32)
    F = np.ascontiguousarray(feat, F32)
    W, H = C.shape[:2]
    eps_a = F32(eps_a)
    hit = F[..., 7] > 0
    a = np.fmax(F[..., 0:3], eps_a)
    with np.errstate(all="ignore"):
        I = np.where(hit[..., None], C / a, C).astype(F32)
        bad = ~(np.isfinite(C).all(axis=-1) & np.isfinite(I).all(axis=-1) & np.isfinite(F).all(axis=-1))
        nx, ny, nz = F[..., 3], F[..., 4], F[..., 5]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = ln > 0
        safe = np.where(ok, ln, F32(1.0))
        N = np.stack([np.where(ok, n / safe, F32(0.0)) for n in (nx, ny, nz)], axis=-1).astype(F32)
        Z = F[..., 6]
        xs, ys = np.arange(W), np.arange(H)
        gx = F32(0.5) * (Z[np.minimum(xs + 1, W - 1), :] - Z[np.maximum(xs - 1, 0), :])
        gy = F32(0.5) * (Z[:, np.minimum(ys + 1, H - 1)] - Z[:, np.maximum(ys - 1, 0)])
        gx = np.where(np.isfinite(gx), gx, F32(0.0))
        gy = np.where(np.isfinite(gy), gy, F32(0.0))
    return I, Z, N, gx.astype(F32), gy.astype(F32), hit, bad, a


def _window(W, H, ox, oy):
    """Slices (p side, q side) of the pixels p whose tap q = p + (ox, oy) lies inside the frame."""
    x0, x1 = max(0, -ox), min(W, W - ox)
    y0, y1 = max(0, -oy), min(H, H - oy)
    if x0 >= x1 or y0 >= y1:
        return None
    return (slice(x0, x1), slice(y0, y1)), (slice(x0 + ox, x1 + ox), slice(y0 + oy, y1 + oy))


def one_pass(I, Z, N, gx, gy, live, step, sc2, sigma_z, eps_z):
    """One a-trous pass; `live` = hit and not bad (the pixels that are filtered and may be taps)."""
    W, H = Z.shape
    sc2, sigma_z, eps_z = F32(sc2), F32(sigma_z), F32(eps_z)
    sum_w = np.zeros((W, H), F32)
    acc = np.zeros((W, H, 3), F32)
    with np.errstate(all="ignore"):
        for dx in range(-2, 3):
            for dy in range(-2, 3):
                win = _window(W, H, step * dx, step * dy)
                if win is None:
                    continue
                p, q = win
                take = live[p] & live[q]
                h = K[abs(dx)] * K[abs(dy)]
                Iq = I[q]
                if dx == 0 and dy == 0:
                    w = np.full(take.shape, h, F32)
                else:
                    Np, Nq = N[p], N[q]
                    wn = np.fmax(F32(0.0), (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2])
                    for _ in range(7):
                        wn = wn * wn
                    gd = gx[p] * F32(step * dx) + gy[p] * F32(step * dy)
                    xz = np.abs(Z[p] - Z[q]) / (sigma_z * np.abs(gd) + eps_z)
                    d = I[p] - Iq
                    xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / sc2
                    w = ((h * wn) * e16(xz)) * e16(xc)
                # a skipped tap adds nothing: the running sums keep their bits
                sum_w[p] = np.where(take, sum_w[p] + w, sum_w[p])
                acc[p] = np.where(take[..., None], acc[p] + w[..., None] * Iq, acc[p])
        out = np.where(live[..., None], acc / np.where(live, sum_w, F32(1.0))[..., None], I)
    return out.astype(F32)


def atrous(color, feat, iterations=5, sigma_c=1.0, sigma_z=1.0, eps_a=1e-2, eps_z=1e-3):
    """The filter of prt_denoise on (W, H, 3) colour and (W, H, 8) features, (W, H, 3) float32."""
    C = np.ascontiguousarray(color, F32)
    I, Z, N, gx, gy, hit, bad, a = prepass(C, feat, eps_a)
    live = hit & ~bad
    for i in range(int(iterations)):
        sc = F32(sigma_c) * (F32(1.0) / F32(1 << i))
        I = one_pass(I, Z, N, gx, gy, live, 1 << i, sc * sc, sigma_z, eps_z)
    with np.errstate(all="ignore"):
        out = np.where(hit[..., None], I * a, I)
    return np.where(bad[..., None], C, out).astype(F32)

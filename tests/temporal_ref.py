"""NumPy float32 restatement of the temporal accumulation (pyrenderer_amd/csrc/prt_denoise.hip:
temporal_kernel, both instantiations) and of the mixed variance select (the in_var branch of var_estimate_kernel).

A helper module like moments_ref.py.  `accumulate(color, feat, cam, prev, ...)` returns what
prt_temporal_accumulate leaves in state, out_color and out_var, with `ids` and `motion` what
prt_temporal_accumulate_motion leaves there, and `atrous_var_mixed(color, feat, in_var, ...)` what
prt_denoise_var_mixed returns, bit for bit.

Camera record: cam[4 i + 0..3] = (side_i, up_i, back_i, E_i) for the world axis i = 0..2; cam[16:19] =
(sw, sh, fd).  A primed name belongs to the previous frame's record.  F = this frame's features (A = F[0:3],
N = F[3:6], Z = F[6]), G = the previous frame's; C = this frame's mean radiance.  With ids: id = ids[p], and the
pixel has a row M = motion[id], a row-major 3 x 4 matrix from this frame's world to the previous one's, when
0 <= id < n_objects.  Any other id has no row and no table entry is read for it; without ids no pixel has one.

per pixel p = (x, y), every operation one f32 operation in this association
 1. hit = F[7] > 0;  a_c = fmax(A_c, eps_a);  I_c = C_c / a_c if hit else C_c
    l = (0.2126 * I_r + 0.7152 * I_g) + 0.0722 * I_b
    bad (a channel of C, I or F is not finite): state = 0, out_color = C, out_var = marker
 2. without history (miss, first frame, any failure below): state = (I, 1, l, l * l, marker, 0)
    marker = the quiet NaN 0x7fc00000
    with ids: a row that holds an entry that is not finite is "no previous pose": this step, before anything
    is projected
 3. u = (x + 0.5) / (W - 1);  v = (y + 0.5) / (H - 1)
    rx = (u - 0.5) * sw / 0.5;  ry = (v - 0.5) * sh / 0.5;  rz = -fd
    f_i = (((rx * side_i + ry * up_i) + rz * back_i) + E_i) - E_i
    ln = sqrt((f_0 * f_0 + f_1 * f_1) + f_2 * f_2)
    X_i = E_i + Z * (f_i / ln)
    with a row: Xp_i = ((M[i][0] * X_0 + M[i][1] * X_1) + M[i][2] * X_2) + M[i][3]
                Np_i = (M[i][0] * N_0 + M[i][1] * N_1) + M[i][2] * N_2;  else Xp = X, Np = N
    rel_i = Xp_i - E'_i;  r = sqrt((rel_0 * rel_0 + rel_1 * rel_1) + rel_2 * rel_2)
    a = (rel_0 * side'_0 + rel_1 * side'_1) + rel_2 * side'_2;  b with up', c with back'
    px = (0.5 + ((0.5 * fd') * a) / (sw' * -c)) * (W - 1) - 0.5;  py with b, sh', H
 4. in range: c < 0 and px > -1 and px < W and py > -1 and py < H (a NaN fails); only then
    x0 = floor(px), fx = px - x0, y0 = floor(py), fy = py - y0
 5. taps q = (x0 + jx, y0 + jy), jx = 0, 1 outer, jy = 0, 1 inner, w = wx[jx] * wy[jy], wx = (1 - fx, fx)
    a tap counts when: inside the frame, h_q > 0, G_q[7] > 0,
        (Np.x * N_q.x + Np.y * N_q.y) + Np.z * N_q.z >= tau_n,
        |G_q[6] - r| <= tau_z * r,
        fmax(fmax(|G_q[0] - F[0]|, |G_q[1] - F[1]|), |G_q[2] - F[2]|) <= tau_a,
        with ids: prev_ids[q] == ids[p] (a plain int32 comparison, ids without a row included)
    sum_w = sum_w + w;  acc_k = acc_k + w * S_q,k for k = I.rgb, h, m1, m2
 6. if sum_w >= w_min: hist = acc / sum_w;  h' = hist.h + 1
        ac = fmax(1 / h', alpha);  am = fmax(1 / h', alpha_m)
        I' = hist.I + ac * (I - hist.I);  m1' = hist.m1 + am * (l - hist.m1);  m2' = hist.m2 + am * (l * l - hist.m2)
 7.     var = fmax(0, m2' - m1' * m1') * ac if h' >= min_history else marker
    else step 2
 8. the one-tap shortcut, per pixel: the two records bytewise equal AND (no row OR the row bytewise
    (1,0,0,0, 0,1,0,0, 0,0,1,0)): the one tap q = p, w = 1, r = Z, Np = N; steps 3 and 4 skipped.  A row that is
    the identity but for a -0 goes the long way
out_color = I' * a if hit else I';  out_var = var

mixed select, per pixel: v = in_var if the pixel is usable (hit and not bad) and in_var is finite and >= 0,
else atrous_var_ref's estimate (0 at a pixel that is not usable).
"""
import numpy as np

import atrous_ref as R
import atrous_var_ref as V

F32 = np.float32
MARKER = np.array([0x7fc00000], np.uint32).view(F32)[0]
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32)
# the parameters the tests pass explicitly (the prototype's set; the library's defaults came out of a sweep later)
DEFAULTS = dict(alpha=0.2, alpha_m=0.2, tau_n=0.9, tau_z=0.02, tau_a=0.05, eps_a=1e-2, min_history=4.0, w_min=0.25)


def prepare(color, feat, eps_a):
    """Step 1: (C, F, hit, a, I, l, bad)."""
    C = np.ascontiguousarray(color, F32)
    F = np.ascontiguousarray(feat, F32)
    with np.errstate(all="ignore"):
        hit = F[..., 7] > 0
        a = np.fmax(F[..., 0:3], F32(eps_a))
        I = np.where(hit[..., None], C / a, C).astype(F32)
        l = V.lum(I).astype(F32)
    bad = ~(np.isfinite(C).all(-1) & np.isfinite(I).all(-1) & np.isfinite(F).all(-1))
    return C, F, hit, a, I, l, bad


def rows_of(ids, motion):
    """(row (W, H, 12), has_row, no_pose, identity) per pixel; pixels without a row get the identity's values,
    which nothing reads."""
    ids = np.asarray(ids, np.int32)
    motion = np.zeros((0, 12), F32) if motion is None else np.ascontiguousarray(motion, F32).reshape(-1, 12)
    n = motion.shape[0]
    has_row = (ids >= 0) & (ids < n)
    table = np.concatenate([motion, IDENTITY[None]])
    row = table[np.where(has_row, ids, n)]
    no_pose = has_row & ~np.isfinite(row).all(-1)
    identity = (row.view(np.uint32) == IDENTITY.view(np.uint32)).all(-1)
    return row, has_row, no_pose, identity


def project(F, cam, prev_cam, row=None, has_row=None):
    """Step 3 and the test of step 4: (px, py, r, in_range, Np), (W, H) arrays and the three planes of Np.
    row, has_row: rows_of's; None when no pixel has a row."""
    W, H = F.shape[:2]
    cam, pc = np.asarray(cam, F32), np.asarray(prev_cam, F32)
    half = F32(0.5)
    x = np.arange(W, dtype=F32)[:, None] + np.zeros((1, H), F32)
    y = np.arange(H, dtype=F32)[None, :] + np.zeros((W, 1), F32)
    wm1, hm1 = F32(W - 1), F32(H - 1)
    with np.errstate(all="ignore"):
        u = (x + half) / wm1
        v = (y + half) / hm1
        rx = (u - half) * cam[16] / half
        ry = (v - half) * cam[17] / half
        rz = -cam[18]
        f = []
        for i in range(3):
            c = cam[4 * i:4 * i + 4]
            f.append((((rx * c[0] + ry * c[1]) + rz * c[2]) + c[3]) - c[3])
        ln = np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
        Xp = [cam[4 * i + 3] + F[..., 6] * (f[i] / ln) for i in range(3)]
        Np = [F[..., 3], F[..., 4], F[..., 5]]
        if row is not None:
            X, N = Xp, Np
            m = [row[..., k] for k in range(12)]
            Xp = [np.where(has_row, ((m[4 * i] * X[0] + m[4 * i + 1] * X[1]) + m[4 * i + 2] * X[2]) + m[4 * i + 3],
                           X[i]).astype(F32) for i in range(3)]
            Np = [np.where(has_row, (m[4 * i] * N[0] + m[4 * i + 1] * N[1]) + m[4 * i + 2] * N[2], N[i]).astype(F32)
                  for i in range(3)]
        rel = [Xp[i] - pc[4 * i + 3] for i in range(3)]
        r = np.sqrt((rel[0] * rel[0] + rel[1] * rel[1]) + rel[2] * rel[2])
        a, b, c = [(rel[0] * pc[k] + rel[1] * pc[4 + k]) + rel[2] * pc[8 + k] for k in range(3)]
        nc = -c
        px = (half + ((half * pc[18]) * a) / (pc[16] * nc)) * wm1 - half
        py = (half + ((half * pc[18]) * b) / (pc[17] * nc)) * hm1 - half
        in_range = (c < 0) & (px > F32(-1.0)) & (px < F32(W)) & (py > F32(-1.0)) & (py < F32(H))
    return px.astype(F32), py.astype(F32), r.astype(F32), in_range, Np


def accumulate(color, feat, cam, prev=None, *, ids=None, motion=None, alpha=0.2, alpha_m=0.2, tau_n=0.9, tau_z=0.02,
               tau_a=0.05, eps_a=1e-2, min_history=4.0, w_min=0.25, diagnostics=False):
    """prt_temporal_accumulate, and with ids prt_temporal_accumulate_motion: (state (W, H, 8), out_color
    (W, H, 3), out_var (W, H)), all float32.  ids: (W, H) int32, or None for no id plane: no pixel has a row and
    no tap is asked for an id.  motion: (n_objects, 12) float32, or None for an empty table.  prev = (state, feat,
    cam) of the previous frame without ids and (state, feat, cam, ids) with them, or None on the first.
    diagnostics=True appends a dict with px, py (the continuous previous pixel), in_range, valid (the history
    was accepted), one_tap (the shortcut of step 8) and no_pose."""
    alpha, alpha_m, tau_n, tau_z, tau_a = F32(alpha), F32(alpha_m), F32(tau_n), F32(tau_z), F32(tau_a)
    min_history, w_min = F32(min_history), F32(w_min)
    C, F, hit, a, I, l, bad = prepare(color, feat, eps_a)
    W, H = l.shape
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.int32)
        assert ids.shape == (W, H)
    one, zero = F32(1.0), F32(0.0)
    new = np.zeros((W, H, 8), F32)
    with np.errstate(all="ignore"):
        new[..., 0:3] = I
        new[..., 3] = one
        new[..., 4] = l
        new[..., 5] = l * l
        new[..., 6] = MARKER
    none = np.zeros((W, H), bool)
    diag = dict(px=None, py=None, in_range=none, valid=none, one_tap=none, no_pose=none)
    if prev is not None:
        S, G, pcam = prev[:3]
        assert len(prev) == (3 if ids is None else 4)
        S = np.ascontiguousarray(S, F32)
        G = np.ascontiguousarray(G, F32)
        cam, pcam = np.asarray(cam, F32), np.asarray(pcam, F32)
        row, has_row, no_pose, identity = (None, none, none, none) if ids is None else rows_of(ids, motion)
        pids = None if ids is None else np.ascontiguousarray(prev[3], np.int32)
        one_tap = (cam.tobytes() == pcam.tobytes()) & (~has_row | identity)
        xi = np.arange(W)[:, None] + np.zeros((1, H), np.int64)
        yi = np.arange(H)[None, :] + np.zeros((W, 1), np.int64)
        with np.errstate(all="ignore"):
            px, py, r, in_range, Np = project(F, cam, pcam, row, has_row)
            px = np.where(one_tap, xi.astype(F32), px)
            py = np.where(one_tap, yi.astype(F32), py)
            r = np.where(one_tap, F[..., 6], r)
            Np = [np.where(one_tap, F[..., 3 + i], Np[i]) for i in range(3)]
            in_range = (in_range | one_tap) & ~no_pose
            fx0 = np.floor(np.where(in_range, px, zero)).astype(F32)
            fy0 = np.floor(np.where(in_range, py, zero)).astype(F32)
            fx, fy = px - fx0, py - fy0
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            wx, wy = (one - fx, fx), (one - fy, fy)
            sw = np.zeros((W, H), F32)
            acc = np.zeros((W, H, 6), F32)
            for jx in (0, 1):
                for jy in (0, 1):
                    qx, qy, w = x0 + jx, y0 + jy, wx[jx] * wy[jy]
                    inside = in_range & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    if jx or jy:
                        inside &= ~one_tap
                    cx, cy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                    Sq, Gq = S[cx, cy], G[cx, cy]
                    nd = (Np[0] * Gq[..., 3] + Np[1] * Gq[..., 4]) + Np[2] * Gq[..., 5]
                    da = np.fmax(np.fmax(np.abs(Gq[..., 0] - F[..., 0]), np.abs(Gq[..., 1] - F[..., 1])),
                                 np.abs(Gq[..., 2] - F[..., 2]))
                    same_id = True if ids is None else pids[cx, cy] == ids
                    take = (inside & same_id & (Sq[..., 3] > 0) & (Gq[..., 7] > 0) & (nd >= tau_n)
                            & (np.abs(Gq[..., 6] - r) <= tau_z * r) & (da <= tau_a))
                    sw = np.where(take, sw + w, sw)
                    acc = np.where(take[..., None], acc + w[..., None] * Sq[..., 0:6], acc)
            valid = hit & ~bad & (sw >= w_min)
            safe = np.where(valid, sw, one)
            hist = acc / safe[..., None]
            nh = hist[..., 3] + one
            ac = np.fmax(one / nh, alpha)
            am = np.fmax(one / nh, alpha_m)
            In = hist[..., 0:3] + ac[..., None] * (I - hist[..., 0:3])
            m1 = hist[..., 4] + am * (l - hist[..., 4])
            m2 = hist[..., 5] + am * (l * l - hist[..., 5])
            var = np.where(nh >= min_history, np.fmax(zero, m2 - m1 * m1) * ac, MARKER)
            blended = np.stack([In[..., 0], In[..., 1], In[..., 2], nh, m1, m2, var, np.zeros((W, H), F32)], -1)
            new = np.where(valid[..., None], blended, new).astype(F32)
        live = hit & ~bad
        diag = dict(px=px, py=py, in_range=in_range & live, valid=valid, one_tap=one_tap & live, no_pose=no_pose & live)
    with np.errstate(all="ignore"):
        out_color = np.where(hit[..., None], new[..., 0:3] * a, new[..., 0:3])
    state = np.where(bad[..., None], zero, new).astype(F32)
    out_color = np.where(bad[..., None], C, out_color).astype(F32)
    out_var = np.where(bad, MARKER, new[..., 6]).astype(F32)
    return (state, out_color, out_var, diag) if diagnostics else (state, out_color, out_var)


def mixed(in_var, estimate, live):
    """var_estimate_kernel with a plane in_var: the variance plane the passes start from."""
    t = np.ascontiguousarray(in_var, F32)
    with np.errstate(all="ignore"):
        return np.where(live & np.isfinite(t) & (t >= 0), t, estimate).astype(F32)


def atrous_var_mixed(color, feat, in_var, iterations=5, sigma_l=1.0, sigma_z=2.0, eps_a=1e-2, eps_z=1e-2, eps_l=1e-2):
    """prt_denoise_var_mixed: ((W, H, 3) image, (W, H) variance actually used), both float32."""
    C = np.ascontiguousarray(color, F32)
    with np.errstate(all="ignore"):   # the set-aside pixels' inf and NaN pass through every step
        I, Z, N, gx, gy, hit, bad, a = R.prepass(C, feat, eps_a)
        live = hit & ~bad
        used = mixed(in_var, V.estimate(I, Z, N, gx, gy, live, sigma_z, eps_z), live)
        Vp = used
        for i in range(int(iterations)):
            I, Vp = V.one_pass(I, Vp, Z, N, gx, gy, live, 1 << i, sigma_l, sigma_z, eps_z, eps_l)
        out = np.where(hit[..., None], I * a, I)
    out = np.where(bad[..., None], C, out).astype(F32)
    return out, used

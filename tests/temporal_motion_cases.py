"""Synthetic two-frame scenes for the tests of the temporal accumulation with per-object motion: a ground plane
and four cards seen from temporal_cases' cameras, features of both frames from float64 ray-plane intersection.

  id 0  ground   the plane z = 0, identity row
  id 1  card     centred at (0.2, 0.1, 0.8), 0.7 x 0.5 half sizes along x and y, normal +z.  Its row M is a rotation
                 of 40 degrees about y composed with 4 degrees about z, both through the card's centre, then a
                 translation of (-0.35, 0.2, -0.1); its previous pose is M applied to its current pose
  id 2  card     a NaN row ("no previous pose"); stands still
  id 3  card     an inf in its translation; stands still
  id 4  card     a row that is the identity but for a -0; stands still

`clean(kind, W, H)` is that scene with a previous state that holds history everywhere; `hostile(kind, W, H)` adds
temporal_cases.hostile's sprinkling of misses, broken depths and colours and edge-of-bound features, ids of -1,
n_objects, 2^31 - 1 and INT_MIN over about 2 % of the pixels each, and previous ids flipped at about 5 %.

A helper module like temporal_cases.py; the CPU tests of the restatement and the GPU tests share it."""
import numpy as np

import temporal_cases as TC

F32 = np.float32
KINDS = TC.KINDS
N_OBJECTS = 5
GROUND, CARD, CARD_NAN, CARD_INF, CARD_NEG0 = range(N_OBJECTS)
ALBEDOS = [TC.ALBEDO, (0.3, 0.6, 0.5), (0.5, 0.3, 0.3), (0.3, 0.3, 0.6), (0.55, 0.55, 0.2)]
CARD_CENTRE = np.array([0.2, 0.1, 0.8])
BAD_IDS = (-1, N_OBJECTS, 2 ** 31 - 1, -2 ** 31)
INF = float("inf")
# (id, centre, half sizes); every card lies in a plane of constant z with its axes along x and y
_RECTS = [(GROUND, (0.0, 0.0, 0.0), (INF, INF)), (CARD, tuple(CARD_CENTRE), (0.7, 0.5)),
          (CARD_NAN, (-0.5, 1.3, 0.3), (0.25, 0.25)), (CARD_INF, (0.5, 1.3, 0.3), (0.25, 0.25)),
          (CARD_NEG0, (0.0, -1.3, 0.3), (0.25, 0.25))]


def card_motion():
    """The 4 x 4 float64 matrix of the moving card: this frame's world to the previous frame's."""
    ay, az = np.radians(40.0), np.radians(4.0)
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = Ry @ Rz
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = CARD_CENTRE - R @ CARD_CENTRE + np.array([-0.35, 0.2, -0.1])
    return M


def motion_table():
    """(N_OBJECTS, 12) float32 rows."""
    rows = np.tile(np.eye(4)[:3].reshape(1, 12), (N_OBJECTS, 1)).astype(F32)
    rows[CARD] = card_motion()[:3].reshape(12)
    rows[CARD_NAN, 5] = np.nan
    rows[CARD_INF, 7] = np.inf
    rows[CARD_NEG0, 1] = -0.0
    return rows


def _surfaces(previous):
    """(id, centre, ex, ey, normal, hx, hy) of every surface in this frame's pose or the previous one."""
    M = card_motion()
    out = []
    for oid, c, (hx, hy) in _RECTS:
        c, ex, ey, n = np.array(c), np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])
        if previous and oid == CARD:
            R = M[:3, :3]
            c, ex, ey, n = R @ c + M[:3, 3], R @ ex, R @ ey, R @ n
        out.append((oid, c, ex, ey, n, hx, hy))
    return out


def features(cam, W, H, previous=False):
    """((W, H, 8) float32 features, (W, H) int32 ids) of the scene from the record `cam`: the closest hit wins, the
    normal is turned toward the ray, a miss has id -1."""
    W, H = int(W), int(H)
    E, d = TC.rays64(cam, W, H)
    if W == 1 or H == 1:   # no pixel-centre ray exists (W - 1 = 0): every pixel looks along the camera's axis
        c = np.asarray(cam, np.float64)
        d = np.broadcast_to(-c[[2, 6, 10]] / np.linalg.norm(c[[2, 6, 10]]), (W, H, 3))
    best = np.full((W, H), np.inf)
    F = np.zeros((W, H, 8), F32)
    ids = np.full((W, H), -1, np.int32)
    for oid, c, ex, ey, n, hx, hy in _surfaces(previous):
        with np.errstate(all="ignore"):
            dn = d @ n
            t = ((c - E) @ n) / dn
            X = E + t[..., None] * d - c
            inside = np.isfinite(t) & (t > 0) & (np.abs(X @ ex) <= hx) & (np.abs(X @ ey) <= hy) & (t < best)
        best = np.where(inside, t, best)
        ids[inside] = oid
        F[inside, 0:3] = np.array(ALBEDOS[oid], F32)
        F[inside, 3:6] = np.where(dn[inside, None] < 0, n, -n).astype(F32)
        F[inside, 6] = t[inside]
        F[inside, 7] = 1
    return F, ids


def clean(kind, W, H, seed=0):
    """(color, feat, cam, ids, motion, prev) without hostile values; prev = (state, feat, cam, ids) holds history at
    every pixel and is None for kind "first"."""
    rng = np.random.default_rng(77 + 1000 * W + 10 * H + seed + KINDS.index(kind))
    cam, pcam = TC.cameras(kind, W, H)
    F, ids = features(cam, W, H)
    C = (rng.random((W, H, 3), dtype=F32) * F32(1.5)) * F[..., 0:3] + F32(0.01)
    if pcam is None:
        return C, F, cam, ids, motion_table(), None
    # the camera that looks away sees nothing: it gets this camera's view of the previous pose, so only c >= 0 rejects
    G, pids = features(cam if kind == "behind" else pcam, W, H, previous=True)
    return C, F, cam, ids, motion_table(), (TC.random_state(rng, W, H), G, pcam, pids)


def hostile(kind, W, H, seed=0):
    """clean() with, sprinkled over its pixels, what temporal_cases.hostile sprinkles and the ids described above."""
    C, F, cam, ids, motion, prev = clean(kind, W, H, seed)
    rng = np.random.default_rng(1000 * W + 10 * H + seed + KINDS.index(kind))
    pick = lambda p: rng.random((W, H)) < p
    m = pick(0.04); F[m, 7] = 0; F[m, 0:7] = 0; ids[m] = -1       # misses
    for v in (1e30, -1e30, np.inf, np.nan, -5.0):
        F[pick(0.02), 6] = v
    for v in (np.nan, np.inf, -np.inf, 3e38):
        C[pick(0.02), rng.integers(0, 3)] = v
    F[pick(0.03), 0] = 1e-4                                         # below eps_a
    F[pick(0.02), 1] = 0.0
    # every surface of this frame faces +z
    m = pick(0.05); F[m, 3:6] = np.array([0.0, 0.5, 0.866], F32)    # normal outside tau_n = 0.9 of (0, 0, 1)
    m = pick(0.05); F[m, 3:6] = np.array([0.0, 0.3, 0.954], F32)    # ... inside
    m = pick(0.05); F[m, 6] *= F32(1.03)                            # depth outside tau_z = 0.02
    m = pick(0.05); F[m, 6] *= F32(1.01)                            # ... inside
    m = pick(0.05); F[m, 2] += F32(0.08)                            # albedo outside tau_a = 0.05
    m = pick(0.05); F[m, 2] += F32(0.03)                            # ... inside
    sprinkled = []
    for v in BAD_IDS:
        m = pick(0.02)
        ids[m] = v
        sprinkled.append((m, v))
    if prev is None:
        return C, F, cam, ids, motion, None
    S, G, pcam, pids = prev
    for m, v in sprinkled:   # half of them stood there before, too: an id without a row still has to agree
        pids[m & pick(0.5)] = v
    m = pick(0.05); G[m, 7] = 0; G[m, 0:7] = 0; pids[m] = -1        # previous misses
    S[pick(0.05), 3] = 0                                            # empty histories
    m = pick(0.02); S[m] = 0; G[m, 6] = np.nan                      # a previous bad pixel: zero state
    m = pick(0.05); pids[m] = (pids[m] + 1) % N_OBJECTS             # another object's id
    return C, F, cam, ids, motion, (S, G, pcam, pids)


def project64(F, cam, prev_cam, M):
    """Float64 continuous previous pixel (px, py) of every first hit carried by the 4 x 4 matrix M."""
    W, H = F.shape[:2]
    E, d = TC.rays64(cam, W, H)
    pc = np.asarray(prev_cam, np.float64)
    X = E + F[..., 6:7].astype(np.float64) * d
    rel = X @ M[:3, :3].T + M[:3, 3] - pc[[3, 7, 11]]
    a, b, c = [rel @ pc[[k, 4 + k, 8 + k]] for k in range(3)]
    with np.errstate(all="ignore"):
        px = (0.5 + 0.5 * pc[18] * a / (pc[16] * -c)) * (W - 1) - 0.5
        py = (0.5 + 0.5 * pc[18] * b / (pc[17] * -c)) * (H - 1) - 0.5
    return px, py

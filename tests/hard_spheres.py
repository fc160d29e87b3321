"""Scenes that are hostile to the sphere and specular side of the kernels, with nothing invalid in
them: many spheres (nested, coincident, tangent, a shell, one around the whole box, one of r = 1e-3),
every material row on a sphere (dielectrics of IOR 1.5, 2.4, exactly 1 and below 1, a mirror, a metal
of roughness 1.5, Lambert rows of both sidedness, an emitter that is no light), dyadic spheres whose
hits, ties and normals are exact, and specks whose f32 normal (p - c) / r is far from unit length.
Shared by tests/test_hard_spheres.py (the oracle alone: the inputs do contain what they are built
for) and tests/test_gpu_hard_spheres.py (the HIP kernels against the oracle's brute-force backend).

Every builder returns a FlatScene that prt_scene_create accepts, made from the Cornell box (or its
triangle soup) by appending material rows and spheres.  Pure NumPy; nothing here knows about the code
under test.
"""
import numpy as np

from hard_scenes import F
from pyrenderer_amd.flatten import FlatScene
from kernel_parity import axis_rays, rays, soup_scene

# rho.rgb, emit, sided, type, ior, roughness (hard_scenes._GREY); albedos inside [2^-40, 2^40], so the
# kernels keep their cheap shading guards (TraceParams::shade_fast) on all of these scenes; the other side,
# and albedos on the bounds themselves, are in tests/shade_cases.py
ROWS = {
    "glass": [0.9, 0.9, 0.9, 0, 0, 3, 1.5, 0],
    "ior2.4": [0.95, 0.9, 0.85, 0, 0, 3, 2.4, 0],
    "ior1": [0.9, 0.95, 0.9, 0, 0, 3, 1.0, 0],
    "ior0.75": [0.85, 0.9, 0.95, 0, 0, 3, 0.75, 0],
    "mirror": [0.9, 0.9, 0.9, 0, 0, 2, 1, 0],
    "rough": [0.8, 0.7, 0.4, 0, 0, 2, 1, 1.5],
    "lambert": [0.6, 0.5, 0.7, 0, 0, 0, 1, 0],
    "lambert1": [0.5, 0.7, 0.6, 0, 1, 0, 1, 0],           # one-sided: the normal is never flipped
    "emitter": [0.3, 0.6, 0.9, 1, 1, 1, 1, 0],             # emits, but lights are triangles: never sampled
}
ROW_NAMES = list(ROWS)

# (centre, radius, row) in index order.  Nothing but the floor-tangent sphere touches a triangle.
ZOO = [
    ((-0.5, 1.55, 0.3), 0.25, "glass"),                    # 0  holds 1
    ((-0.45, 1.5, 0.3), 0.17, "ior2.4"),                   # 1  nested in 0
    ((0.5, 1.6, -0.3), 0.2, "mirror"),                     # 2  coincident with 3: never wins
    ((0.5, 1.6, -0.3), 0.2, "lambert"),                    # 3
    ((-0.55, 0.25, 0.6), 0.15, "rough"),                   # 4  tangent to 5 at x = -0.4
    ((-0.25, 0.25, 0.6), 0.15, "lambert1"),                # 5
    ((0.45, 1.0, -0.55), 0.30, "glass"),                   # 6  shell: 7 is 0.01 inside it
    ((0.45, 1.0, -0.55), 0.29, "ior0.75"),                 # 7
    ((0.0, 1.0, 2.5), 5.0, "ior1"),                        # 8  around the whole box and the Cornell camera
    ((0.7, 0.15, -0.3), 0.15, "lambert"),                  # 9  rests on the floor, tangent at y = 0
    ((0.0, 1.5, 0.6), 1e-3, "lambert"),                    # 10 the small one
    ((-0.35, 1.4, -0.3), 0.15, "emitter"),                 # 11 above the tall box
    ((0.35, 0.85, 0.4), 0.2, "ior2.4"),                    # 12 above the short box
    ((-0.7, 0.9, 0.7), 0.18, "mirror"),                    # 13
]
ZOO_COINCIDENT = (2, 3)
ZOO_SMALL = 10
ZOO_IOR24 = (1, 12)

# dyadic centres and radii: every operation of sphere_hit and of (p - c) / r is exact on the axis rays
DYADIC = [
    ((0.5, 0.25, -0.5), 0.25, "mirror"),                   # 0  coincident with 1, tangent to the floor
    ((0.5, 0.25, -0.5), 0.25, "lambert"),                  # 1
    ((-0.5, 0.5, 0.5), 0.25, "lambert"),                   # 2
]
DYADIC_CENTRES = ((1, DYADIC[1]), (2, DYADIC[2]))          # (winning sphere index, sphere) per distinct centre

SPECKS = ((1e-3, 200.0), (1e-4, 2000.0), (1e-4, 2.0))     # (radius, distance of the ray origins)
SPECK_CENTRE = (0.1, 1.0, 0.2)
N_MANY = 67                                                # a loop length that is no multiple of anything


def with_spheres(flat, spheres):
    """`flat` plus every row of ROWS (appended to its material table) and the given spheres."""
    n_mat = flat.mat.shape[0]
    mat = np.concatenate([flat.mat, np.array([ROWS[k] for k in ROW_NAMES], F)])
    sph = np.array([[*c, r] for c, r, _ in spheres], np.float64).astype(F)
    sph_mat = np.array([n_mat + ROW_NAMES.index(row) for _, _, row in spheres], np.int32)
    lo, hi = sph[:, :3] - sph[:, 3:], sph[:, :3] + sph[:, 3:]
    return FlatScene(flat.tri_v, flat.tri_n, flat.tri_mat, flat.tri_prim, np.concatenate([flat.prim_lo, lo]),
                     np.concatenate([flat.prim_hi, hi]), mat, flat.light_tri, flat.light_off, flat.direct_rgb,
                     sph, sph_mat)


def inside_rays(flat, n, seed):
    """n rays whose origins are drawn uniformly inside the scene's spheres, taking the spheres in turn
    (ray i starts in sphere i % n_sph), with unit directions as rays draws them: the first hit is the
    far root of the sphere itself unless something lies inside it.  Returns (o, d)."""
    rng = np.random.default_rng(seed)
    sph = flat.sph.astype(np.float64)[np.arange(n) % flat.sph.shape[0]]
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return (sph[:, :3] + 0.999 * sph[:, 3:] * v).astype(F), rays(n, seed + 1)[1]


def many_spheres(seed=5):
    rng = np.random.default_rng(seed)
    c = rng.uniform((-0.85, 0.15, -0.85), (0.85, 1.85, 0.85), (N_MANY, 3))
    r = rng.uniform(0.02, 0.15, N_MANY)
    rows = rng.integers(0, len(ROW_NAMES), N_MANY)
    return [(tuple(c[k]), float(r[k]), ROW_NAMES[rows[k]]) for k in range(N_MANY)]


def dyadic_rays():
    """The axis rays of the dyadic scene: for each distinct centre and each of +-x, +-y, +-z a 17 x 17 grid
    of origins (steps of r / 8 over the sphere's cross-section), once from 0.5 before the centre plane
    ("above": the near root, or a pass beside the sphere) and once on the centre plane itself ("centre":
    the far root from inside).  Returns {set: (o, d, meta)}; meta is an (n, 5) int array of (winning
    sphere index, axis, sign, iu, iv) with iu = iv = 8 on the sphere's own axis."""
    out = {}
    g = np.arange(17)
    iu, iv = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    for kind, back in (("above", 0.5), ("centre", 0.0)):
        oo, dd, mm = [], [], []
        for win, (c, r, _) in DYADIC_CENTRES:
            for axis in range(3):
                for sign in (1.0, -1.0):
                    o = np.tile(np.array(c, np.float64), (iu.size, 1))
                    o[:, (axis + 1) % 3] += (iu - 8) * (r / 8)
                    o[:, (axis + 2) % 3] += (iv - 8) * (r / 8)
                    o[:, axis] -= sign * back
                    d = np.zeros((iu.size, 3))
                    d[:, axis] = sign
                    oo.append(o)
                    dd.append(d)
                    mm.append(np.stack([np.full(iu.size, win), np.full(iu.size, axis),
                                        np.full(iu.size, int(sign)), iu, iv], 1))
        out[kind] = (np.concatenate(oo).astype(F), np.concatenate(dd).astype(F), np.concatenate(mm))
    return out


def speck_rays(radius, distance, n=4096, seed=0):
    """Rays aimed at the speck from `distance` away through the box's open front: direction (0, 0, -1) plus
    N(0, 0.05) in x and y, normalised; through the centre plus N(0, radius / 2); origin and direction in
    float64, rounded once."""
    rng = np.random.default_rng(900 + seed)
    d = np.concatenate([rng.normal(0, 0.05, (n, 2)), -np.ones((n, 1))], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aim = np.array(SPECK_CENTRE) + rng.normal(0, radius / 2, (n, 3))
    return (aim - d * distance).astype(F), d.astype(F)


def speck_name(radius, distance):
    return "specks-%g-%g" % (radius, distance)


# ------------------------------------------------------------------ the catalogue both test files walk
CASES = ["zoo", "dyadic"] + [speck_name(r, d) for r, d in SPECKS] + ["soup-zoo", "many"]
_cache = {}


def case(cornell, name):
    """(flat, {ray set: (o, d)}) of one catalogue entry; `cornell` is the session fixture.  Built once
    per process and not modified by its users.
      zoo            the box + ZOO: 4096 interior rays, 2048 inside-origin rays, the axis-aligned set
      dyadic         the box + DYADIC: the "above" and "centre" grids of dyadic_rays (3468 rays each)
      specks-R-D     the box + one Lambert sphere of radius R: 4096 rays from D away
      soup-zoo       soup_scene(cornell, 300, 9) + ZOO (not LDS-resident): interior and inside-origin
      many           the box + 67 random spheres: 4096 interior rays"""
    if name in _cache:
        return _cache[name]
    box = cornell[2]
    if name == "zoo":
        flat = with_spheres(box, ZOO)
        sets = {"interior": rays(4096, 61), "inside": inside_rays(flat, 2048, 62), "axis": axis_rays(100, 63)}
    elif name == "dyadic":
        flat = with_spheres(box, DYADIC)
        sets = {k: v[:2] for k, v in dyadic_rays().items()}
    elif name.startswith("specks-"):
        r, dist = (float(x) for x in name.split("-", 1)[1].rsplit("-", 1))
        flat = with_spheres(box, [(SPECK_CENTRE, r, "lambert")])
        sets = {"aimed": speck_rays(r, dist)}
    elif name == "soup-zoo":
        flat = with_spheres(soup_scene(cornell, 300, 9), ZOO)
        sets = {"interior": rays(4096, 64), "inside": inside_rays(flat, 2048, 65)}
    elif name == "many":
        flat, sets = with_spheres(box, many_spheres()), {"interior": rays(4096, 66)}
    else:
        raise KeyError(name)
    _cache[name] = (flat, sets)
    return _cache[name]

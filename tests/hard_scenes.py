"""Scenes and rays that are hostile to a BVH traversal, with nothing invalid in them: exact ties
(a dyadic lattice, coincident quads), needle and degenerate triangles, similarity placements of a
scene far from the origin and at other scales, and rays that start far outside the scene.  Shared by
tests/test_hard_scenes.py (the oracle alone: the inputs do contain what they are built for) and
tests/test_gpu_hard_hits.py (the HIP traversal against the oracle's brute-force backend).

Every builder returns a FlatScene that prt_scene_create accepts: at least one light, valid material
ids, unit normals ((0, 1, 0) for a triangle without area).  Pure NumPy; only `tie_rays` asks the
oracle, and nothing here knows about the code under test.
"""
import numpy as np

from oracle import oracle as O
from pyrenderer_amd.flatten import FlatScene
import kernel_parity as KP
from kernel_parity import T_MAX, T_MIN, random_bounds  # noqa: F401  (random_bounds: re-exported)

F = np.float32
_GREY = [0.5, 0.5, 0.5, 0, 0, 0, 1, 0]         # rho.rgb, emit, sided, type, ior, roughness
_EMIT = [1, 1, 1, 1, 1, 1, 1, 0]               # the Cornell light's row

PLACEMENTS = [(2.0 ** -10, (0.0, 0.0, 0.0)), (2.0 ** 10, (0.0, 0.0, 0.0)), (1.0, (1000.0, -2000.0, 500.0)),
              (370.0, (1e4, 3e3, -2e4)), (2.0 ** -10, (1.0, 1.0, 1.0))]
FAR_EXTENTS = (100.0, 1000.0)
LATTICE_DIRS = ((0.0, 0.0, -1.0), (0.0, 0.0, -2.0), (0.25, 0.0, -1.0), (0.125, -0.25, -1.0))


def _unit_normals(tri_v):
    """Face normals in float64, rounded once; (0, 1, 0) where the triangle has no area."""
    v = np.asarray(tri_v, F).reshape(-1, 3, 3).astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(n, axis=1)
    out = np.tile([0.0, 1.0, 0.0], (v.shape[0], 1))
    ok = ln > 0
    out[ok] = n[ok] / ln[ok, None]
    return out.astype(F)


def _tri_bounds(tri_v):
    v = np.asarray(tri_v, F).reshape(-1, 3, 3)
    return v.min(1), v.max(1)


def _per_triangle(tri_v, tri_n, tri_mat, mat, lights, direct_rgb):
    """FlatScene with one primitive per triangle; `lights` is a list of triangle-id lists."""
    tri_v = np.asarray(tri_v, F).reshape(-1, 9)
    lo, hi = _tri_bounds(tri_v)
    light_tri = np.concatenate([np.asarray(l, np.int32) for l in lights])
    light_off = np.concatenate([[0], np.cumsum([len(l) for l in lights])]).astype(np.int32)
    return FlatScene(tri_v, tri_n, tri_mat, np.arange(tri_v.shape[0], dtype=np.int32), lo, hi, mat, light_tri,
                     light_off, direct_rgb)


def _lights(flat):
    return [flat.light_tri[flat.light_off[k]:flat.light_off[k + 1]] for k in range(flat.n_light)]


def reindexed(flat, perm):
    """The same scene with triangle perm[i] at index i (lights follow their triangles)."""
    perm = np.asarray(perm, np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.shape[0])
    return _per_triangle(flat.tri_v[perm], flat.tri_n[perm], flat.tri_mat[perm], flat.mat,
                         [inv[l] for l in _lights(flat)], flat.direct_rgb)


def _with_extras_first(flat, tv):
    """`tv` (m, 9) in front of the scene's own triangles, as one more primitive of material 0
    (the layout of kernel_parity.soup_scene: the light's triangle ids move)."""
    tv = np.asarray(tv, F).reshape(-1, 9)
    m = tv.shape[0]
    lo, hi = _tri_bounds(tv)
    return FlatScene(np.concatenate([tv, flat.tri_v]), np.concatenate([_unit_normals(tv), flat.tri_n]),
                     np.concatenate([np.zeros(m, np.int32), flat.tri_mat]),
                     np.concatenate([np.zeros(m, np.int32), flat.tri_prim + 1]),
                     np.concatenate([lo.min(0)[None], flat.prim_lo]), np.concatenate([hi.max(0)[None], flat.prim_hi]),
                     flat.mat, flat.light_tri + m, flat.light_off, flat.direct_rgb)


def scene_box(flat):
    """(centre, largest extent) of the scene's vertices, float64."""
    v = flat.tri_v.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return (lo + hi) / 2, float((hi - lo).max())


# ------------------------------------------------------------------ lattice
def _to_world(local, axis):
    """Local (u, v, w) -> world: w on `axis`, u and v on the two axes after it (cyclic)."""
    out = np.zeros_like(local)
    out[..., (axis + 1) % 3] = local[..., 0]
    out[..., (axis + 2) % 3] = local[..., 1]
    out[..., axis] = local[..., 2]
    return out


def _lattice_local(cells=8):
    """cells x cells cells over [-1, 1]^2, two triangles each, then the light's two."""
    w = 2.0 / cells
    tris = []
    for j in range(cells):
        for i in range(cells):
            u0, v0 = -1 + w * i, -1 + w * j
            u1, v1 = u0 + w, v0 + w
            tris.append([[u0, v0, 0], [u1, v0, 0], [u1, v1, 0]])
            tris.append([[u0, v0, 0], [u1, v1, 0], [u0, v1, 0]])
    tris.append([[-0.5, -0.5, 2], [0.5, 0.5, 2], [0.5, -0.5, 2]])     # the light, facing the lattice
    tris.append([[-0.5, -0.5, 2], [-0.5, 0.5, 2], [0.5, 0.5, 2]])
    return np.array(tris, np.float64)


def lattice(axis):
    """An 8 x 8 grid of 0.25-wide cells, two triangles per cell, in the plane x, y or z = 0 over
    [-1, 1]^2, and a two-triangle light at height 2.  All coordinates are dyadic, so for the ray set
    every product and sum of Moeller-Trumbore is exact in f32 and ties are real ones.

    Returns (flat, rays); rays holds one (o, d, expected_id, n_candidates) per direction of
    LATTICE_DIRS (permuted to the axis, not normalised) from the 17 x 17 half-cell grid at height 1.
    expected_id is decided in float64: the lowest index among the triangles whose closed set holds
    the hit point, -1 where the ray leaves the lattice; n_candidates counts those triangles."""
    loc = _lattice_local()
    tv = _to_world(loc, axis).reshape(-1, 9)
    n = tv.shape[0]
    mat = np.array([_GREY, _EMIT], F)
    tri_mat = np.zeros(n, np.int32)
    tri_mat[-2:] = 1
    flat = _per_triangle(tv, _unit_normals(tv), tri_mat, mat, [[n - 2, n - 1]], [0.9, 0.85, 0.7])
    g = -1 + 0.125 * np.arange(17)
    uu, vv = np.meshgrid(g, g, indexing="ij")
    o_loc = np.stack([uu.ravel(), vv.ravel(), np.ones(uu.size)], 1)
    return flat, _lattice_rays(loc[:128], o_loc, axis)


def _lattice_rays(loc, o_loc, axis):
    """One (o, d, expected_id, n_candidates) per direction of LATTICE_DIRS from the local origins `o_loc` at
    height 1 over the lattice triangles `loc` (without the light), decided in float64."""
    a, b, c = loc[:, 0, :2], loc[:, 1, :2], loc[:, 2, :2]

    def cross2(p, q):
        return p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]

    rays = []
    for dl in LATTICE_DIRS:
        dl = np.array(dl, np.float64)
        p = (o_loc + dl * (-1.0 / dl[2]))[:, None, :2]               # (rays, 1, 2), exact
        # closed-set membership by the three edge functions (counter-clockwise triangles), exact too
        inside = ((cross2(b - a, p - a) >= 0) & (cross2(c - b, p - b) >= 0) & (cross2(a - c, p - c) >= 0))
        cand = inside.sum(1)
        expect = np.where(cand > 0, inside.argmax(1), -1).astype(np.int64)
        rays.append((_to_world(o_loc, axis).astype(F), np.tile(_to_world(dl, axis), (o_loc.shape[0], 1)).astype(F),
                     expect, cand))
    return rays


N_LATTICE_SMALL_RAYS = 4096
_ROWS3 = [[0.9, 0.15, 0.15, 0, 0, 0, 1, 0], [0.15, 0.9, 0.15, 0, 0, 0, 1, 0], [0.15, 0.15, 0.9, 0, 0, 0, 1, 0]]


def lattice_small(axis, cells=4):
    """The dyadic lattice small enough for the LDS-resident kernels: cells x cells cells (4: of width 0.5,
    32 triangles) and the two-triangle light at height 2, with a material per triangle: three diffuse rows
    of clearly different albedo, tri_mat[i] = i % 3, and the emitter on the light.  The two triangles of a
    cell and most neighbours across a cell edge differ in material, so the winner of a tie changes the
    path's radiance, not only the id.

    Returns (flat, (o, d, expected_id, n_candidates)): the (2 cells + 1)^2 half-cell origins at height 1 for
    each direction of LATTICE_DIRS, one direction after the other, tiled to 4096 rays (a caller ray's path
    is drawn by its index, so a repeated ray is another path); expected_id as lattice() decides it."""
    loc = _lattice_local(cells)
    tv = _to_world(loc, axis).reshape(-1, 9)
    n = tv.shape[0]
    mat = np.array(_ROWS3 + [_EMIT], F)
    tri_mat = (np.arange(n) % 3).astype(np.int32)
    tri_mat[-2:] = 3
    flat = _per_triangle(tv, _unit_normals(tv), tri_mat, mat, [[n - 2, n - 1]], [0.9, 0.85, 0.7])
    g = -1 + (1.0 / cells) * np.arange(2 * cells + 1)
    uu, vv = np.meshgrid(g, g, indexing="ij")
    o_loc = np.stack([uu.ravel(), vv.ravel(), np.ones(uu.size)], 1)
    rays = _lattice_rays(loc[:-2], o_loc, axis)
    idx = np.arange(N_LATTICE_SMALL_RAYS) % (len(rays) * o_loc.shape[0])
    return flat, tuple(np.concatenate([r[k] for r in rays])[idx] for k in range(4))


# ------------------------------------------------------------------ layers
def layers(cornell_flat, K=6, seed=0):
    """The Cornell box with its floor quad K times at the identical position (2 K coincident
    triangles: more than a leaf of four holds), successive copies with different materials, one of
    them an emitter that is also a light; some twenty small filler triangles just above the floor;
    the index order shuffled by `seed`, so which copy has the lowest id differs per seed and the
    copies land in different leaves."""
    f = cornell_flat
    rng = np.random.default_rng(1000 + seed)
    emitter = f.mat.shape[0]
    mat = np.concatenate([f.mat, np.array([[0.3, 0.6, 0.9, 1, 1, 1, 1, 0]], F)])
    copy_mats = [3, 4, emitter, 5, 6, 3, 4]
    tv, tm, lights = [f.tri_v], [f.tri_mat], _lights(f)
    n = f.n_tri
    for k in range(K - 1):
        tv.append(f.tri_v[0:2])
        tm.append(np.full(2, copy_mats[k % len(copy_mats)], np.int32))
        if copy_mats[k % len(copy_mats)] == emitter:
            lights = lights + [np.array([n, n + 1])]
        n += 2
    frng = np.random.default_rng(77)                                   # the same fillers for every seed
    c = np.stack([frng.uniform(-0.9, 0.9, 20), frng.uniform(0.02, 0.3, 20), frng.uniform(-0.9, 0.9, 20)], 1)
    fill = (c[:, None, :] + frng.normal(0, 0.04, (20, 3, 3))).astype(F).reshape(-1, 9)
    tv.append(fill)
    tm.append(np.zeros(20, np.int32))
    tv = np.concatenate(tv)
    tn = np.concatenate([f.tri_n, np.tile(f.tri_n[0:2], (K - 1, 1)), _unit_normals(fill)])
    whole = _per_triangle(tv, tn, np.concatenate(tm), mat, lights, f.direct_rgb)
    return reindexed(whole, rng.permutation(whole.n_tri))


# ------------------------------------------------------------------ slivers
N_NEEDLES = 32


def slivers(cornell_flat, width, n_needles=N_NEEDLES, n_each=8):
    """The Cornell box plus, first in index order: 32 needles of length 0.4 and the given width,
    8 point triangles, 8 collinear ones, 8 of extent 1e-6, and one triangle larger than the whole
    box in the plane z = -1.5 behind the back wall.  (93 triangles are more than the LDS-resident
    kernels hold; n_needles = 8, n_each = 2 gives the same mixture in 51.)

    Returns (flat, (o, d)): 4096 rays from interior origins aimed at Dirichlet(1, 1, 1) points of
    the needles (ids 0 .. n_needles - 1), then 8000 random interior rays."""
    rng = np.random.default_rng(4242)
    # in the free space above the two boxes (the tall one ends at y = 1.2), pointing mostly sideways
    base = np.stack([rng.uniform(-0.55, 0.55, n_needles), rng.uniform(1.3, 1.8, n_needles),
                     rng.uniform(-0.55, 0.55, n_needles)], 1)
    along = rng.normal(size=(n_needles, 3)) * [1.0, 0.3, 1.0]
    along /= np.linalg.norm(along, axis=1, keepdims=True)
    side = np.cross(along, rng.normal(size=(n_needles, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    needles = np.stack([base - 0.5 * width * side, base + 0.5 * width * side, base + 0.4 * along], 1)
    pt = np.stack([rng.uniform(-0.8, 0.8, n_each), rng.uniform(0.2, 1.8, n_each), rng.uniform(-0.8, 0.8, n_each)], 1)
    points = np.repeat(pt[:, None, :], 3, axis=1)
    c0 = np.round(rng.uniform(-0.75, 0.75, (n_each, 3)) * 64) / 64 + [0, 1, 0]        # dyadic: exactly collinear
    step = np.round(rng.uniform(-0.1, 0.1, (n_each, 3)) * 64) / 64 + 1.0 / 64
    collinear = np.stack([c0, c0 + step, c0 + 2 * step], 1)
    tc = np.stack([rng.uniform(-0.8, 0.8, n_each), rng.uniform(0.2, 1.8, n_each), rng.uniform(-0.8, 0.8, n_each)], 1)
    tiny = tc[:, None, :] + rng.uniform(-0.5e-6, 0.5e-6, (n_each, 3, 3))
    huge = np.array([[[-6.0, -3.0, -1.5], [6.0, -3.0, -1.5], [0.0, 8.0, -1.5]]])
    extras = np.concatenate([needles, points, collinear, tiny, huge]).astype(F).reshape(-1, 9)
    flat = _with_extras_first(cornell_flat, extras)
    # aimed rays: the target is a point of the f32 needle, the direction normalised in float64
    n_aim = 4096
    k = rng.integers(0, n_needles, n_aim)
    w = rng.dirichlet([1.0, 1.0, 1.0], n_aim)
    target = np.einsum("nk,nkc->nc", w, extras[:n_needles].reshape(-1, 3, 3)[k].astype(np.float64))
    o = rng.uniform((-0.95, 0.05, -0.95), (0.95, 1.95, 0.95), (n_aim, 3)).astype(F)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    ro, rd = KP.rays(8000, 31)
    return flat, (np.concatenate([o, ro]), np.concatenate([d, rd]))


# ------------------------------------------------------------------ placements and far rays
def placed(flat, scale, translate):
    """Similarity transform x -> scale * x + translate of a scene without spheres, evaluated in
    float64 and rounded once to f32 (vertices and primitive bounds; normals are unchanged)."""
    assert flat.sph.shape[0] == 0
    t = np.asarray(translate, np.float64)

    def xf(a):
        return (a.astype(np.float64).reshape(-1, 3) * scale + t).astype(F)

    return FlatScene(xf(flat.tri_v).reshape(-1, 9), flat.tri_n, flat.tri_mat, flat.tri_prim, xf(flat.prim_lo),
                     xf(flat.prim_hi), flat.mat, flat.light_tri, flat.light_off, flat.direct_rgb)


def placed_points(o, scale, translate):
    """Ray origins of the unit Cornell box mapped into the placed one."""
    return (np.asarray(o, np.float64) * scale + np.asarray(translate, np.float64)).astype(F)


def far_rays(flat, n, seed, extents=FAR_EXTENTS[0]):
    """n rays with unit directions as kernel_parity.rays draws them, from origins
    centre - d * D + a jitter of a quarter extent, D = min(extents * extent, 0.4 * T_MAX): the hits
    stay below the reference's t_max of 99999.9.  Returns (o, d, D)."""
    centre, extent = scene_box(flat)
    D = min(extents * extent, 0.4 * float(T_MAX))
    _, d = KP.rays(n, seed)
    rng = np.random.default_rng(seed + 500)
    o = centre - d.astype(np.float64) * D + rng.uniform(-0.25, 0.25, (n, 3)) * extent
    return o.astype(F), d, D


def placement_rays(flat, scale, translate, n=6000, seed=0):
    """The ray sets of one placed scene: {name: (o, d)} with interior rays, the axis-aligned set
    (direction components of exactly +-0) and far rays at both distances."""
    o, d = KP.rays(n, 40 + seed)
    ao, ad = KP.axis_rays(250, 41 + seed)
    sets = {"interior": (placed_points(o, scale, translate), d), "axis": (placed_points(ao, scale, translate), ad)}
    for e in FAR_EXTENTS:
        fo, fd, _ = far_rays(flat, n, 42 + seed, e)
        sets["far%d" % e] = (fo, fd)
    return sets


# ------------------------------------------------------------------ ties
def tie_rays(flat, o, d):
    """Mask of the rays whose brute-force winner changes when the triangle order is reversed: rays
    that end on two triangles with bit-equal t.  The oracle alone."""
    n = flat.n_tri
    hit, _, tri, _ = O.OracleScene.from_flat(flat).closest(o, d, T_MIN, T_MAX)
    rhit, _, rtri, _ = O.OracleScene.from_flat(reindexed(flat, np.arange(n)[::-1])).closest(o, d, T_MIN, T_MAX)
    assert np.array_equal(hit, rhit)
    return (hit != 0) & (tri != n - 1 - rtri)


# ------------------------------------------------------------------ the catalogue both test files walk
AXES = "xyz"
CASES = (["lattice-%s" % a for a in AXES] + ["layers-%d" % s for s in range(3)]
         + ["slivers-1e-3", "slivers-1e-5", "slivers8-1e-5"]
         + ["cornell"] + ["%s-p%d" % (b, k) for b in ("soup", "box") for k in range(len(PLACEMENTS))])
_cache = {}


def case(cornell, name):
    """(flat, {ray set: (o, d)}) of one catalogue entry; `cornell` is the session fixture.  Built
    once per process and not modified by its users.
      lattice-x|y|z    one ray set per direction of LATTICE_DIRS
      layers-0|1|2     20 000 interior rays
      slivers-W        the 4096 aimed + 8000 random rays
      slivers8-W       the same with 8 needles and 2 of each degenerate kind (51 triangles)
      cornell          the plain box: 20 000 interior rays, 20 000 far rays at each distance
      soup-pK, box-pK  placement K of soup_scene(cornell, 300, 9) / of the plain box: interior,
                       axis-aligned and far rays at each distance"""
    if name in _cache:
        return _cache[name]
    kind, _, arg = name.partition("-")
    box = cornell[2]
    if kind == "lattice":
        flat, rays = lattice(AXES.index(arg))
        sets = {"dir%d" % k: (o, d) for k, (o, d, _, _) in enumerate(rays)}
    elif kind == "layers":
        flat, sets = layers(box, 6, int(arg)), {"interior": KP.rays(20000, 1)}
    elif kind in ("slivers", "slivers8"):
        flat, rays = slivers(box, float(arg)) if kind == "slivers" else slivers(box, float(arg), 8, 2)
        sets = {"aimed+random": rays}
    elif kind == "cornell":
        flat, sets = box, {"interior": KP.rays(20000, 1)}
        for e in FAR_EXTENTS:
            sets["far%d" % e] = far_rays(box, 20000, 7, e)[:2]
    else:
        scale, translate = PLACEMENTS[int(arg[1:])]
        flat = placed(KP.soup_scene(cornell, 300, 9) if kind == "soup" else box, scale, translate)
        sets = placement_rays(flat, scale, translate)
    _cache[name] = (flat, sets)
    return _cache[name]

"""Cornell boxes whose material table or face normals put the shading quotients on their guarded side,
with nothing invalid in them: a black wall, a pure red one, albedo channels of 1e-20, 1e-40 (an f32
denormal) and one ulp below 2^-40, a light whose colour has zero channels, face normals of length 3 and
0.25, and an albedo of 2^41 whose throughput overflows; and the boundary of the other side: an albedo of
exactly 2^-40 or 2^40, normals of length exactly 2 or 0.5.  The host classifies a scene by exactly these
bounds (every albedo channel in [2^-40, 2^40], every face normal's length in [0.5, 2]:
TraceParams::shade_fast), and the LDS trace kernels divide the Lambert weight and the NEE term under a
cheap wave-level guard only where the flag is set; every other scene takes the full division with the
reference's pdf = 1e-4 NaN rule.  Shared by tests/test_shade_cases.py (the host's classification and the
oracle alone: the inputs do contain what they are built for) and tests/test_gpu_shade_cases.py (the HIP
kernels against the oracle).

The host measures a normal's squared length in float64, and the f32 normals of the rotated boxes' side
faces come to 1 + 3.7e-8 and 1 + 5.6e-8.  Twice such a normal is longer than 2, so n3's triangles x 2
(`n2-over`) sit just outside the bound, on the guarded side; `n2` doubles only those of n3's triangles
whose length is exactly 1 (walls, box tops, the light), which puts it exactly on the bound.  Half of
every one of them is still >= 0.5, so `n-half` scales all of n3's triangles.

Every builder takes the Cornell box's FlatScene and returns a new one in which only `mat` or `tri_n` is
replaced.  Pure NumPy; nothing here knows about the code under test.
"""
import numpy as np

from pyrenderer_amd.flatten import FlatScene
import kernel_parity as KP

F = np.float32
N_RAYS, DEPTH, SEED = 4096, 8, 17          # the first 4096 of rays(4096, 3), traced at depth 8 with seed 17

# material rows of the Cornell box: 0 floor, 1 ceiling, 2 back wall, 3 the green wall, 4 the red wall, 5 and 6
# the two boxes, 7 the light (test_shade_cases.py checks the ones named here against the geometry)
FLOOR, BACK, RED_WALL, LIGHT = 0, 2, 4, 7
CHANNEL = 1                                 # the channel of the floor's albedo that the one-channel cases set
LO, HI = F(2.0 ** -40), F(2.0 ** 40)        # the bounds of the host's albedo test, both inside
N3_EVERY, NQ_EVERY = 3, 5


def _replaced(flat, mat=None, tri_n=None):
    return FlatScene(flat.tri_v, flat.tri_n if tri_n is None else np.ascontiguousarray(tri_n, F), flat.tri_mat,
                     flat.tri_prim, flat.prim_lo, flat.prim_hi, flat.mat if mat is None else np.ascontiguousarray(mat, F),
                     flat.light_tri, flat.light_off, flat.direct_rgb)


def with_row(flat, row, rho):
    """The scene with material row `row`'s albedo replaced by `rho` (three channels)."""
    mat = flat.mat.copy()
    mat[row, :3] = np.asarray(rho, F)
    return _replaced(flat, mat=mat)


def with_channel(flat, value, row=FLOOR, channel=CHANNEL):
    """The scene with one albedo channel replaced by the f32 `value`."""
    mat = flat.mat.copy()
    mat[row, channel] = F(value)
    return _replaced(flat, mat=mat)


def scaled_triangles(flat, every):
    """Ids of the triangles whose normal the n-cases scale: the `every`-th, the 2 `every`-th and so on
    (ids every - 1, 2 every - 1, ...), which in the box and in its soup reach the light's last triangle."""
    return np.arange(every - 1, flat.n_tri, every)


def exactly_unit(flat):
    """Mask of the triangles whose f32 normal has a squared length of exactly 1 in float64 (the box's
    axis-aligned faces; the rotated boxes' side faces come to 1 + 3.7e-8 and 1 + 5.6e-8)."""
    n = flat.tri_n.astype(np.float64)
    return (n * n).sum(1) == 1.0


def with_normals(flat, every, scale, unit_only=False):
    """The scene with every `every`-th triangle's face normal multiplied by the f32 `scale` (in f32;
    exact for a power of two), with `unit_only` only those of them whose length is exactly 1."""
    ids = scaled_triangles(flat, every)
    if unit_only:
        ids = ids[exactly_unit(flat)[ids]]
    tri_n = flat.tri_n.copy()
    tri_n[ids] *= F(scale)
    return _replaced(flat, tri_n=tri_n)


# name -> (builder, plain, shade_fast, the oracle's radiance stays finite)
TABLE = {
    # the guarded side
    "black": (lambda f: with_row(f, BACK, (0, 0, 0)), True, False, True),
    "red": (lambda f: with_row(f, RED_WALL, (1, 0, 0)), True, False, True),
    "tiny": (lambda f: with_channel(f, 1e-20), True, False, True),
    "denormal": (lambda f: with_channel(f, 1e-40), True, False, True),
    "below": (lambda f: with_channel(f, np.nextafter(LO, F(0))), True, False, True),
    "red-light": (lambda f: with_row(f, LIGHT, (1, 0, 0)), True, False, True),
    "n3": (lambda f: with_normals(f, N3_EVERY, 3), True, False, True),
    "n-quarter": (lambda f: with_normals(f, NQ_EVERY, 0.25), True, False, True),
    "n2-over": (lambda f: with_normals(f, N3_EVERY, 2), True, False, True),
    "above": (lambda f: with_channel(f, 2.0 ** 41), True, False, False),
    # the boundary of the fast side
    "lo-edge": (lambda f: with_channel(f, LO), True, True, True),
    "n2": (lambda f: with_normals(f, N3_EVERY, 2, unit_only=True), True, True, True),
    "n-half": (lambda f: with_normals(f, N3_EVERY, 0.5), True, True, True),
    "hi-edge": (lambda f: with_channel(f, HI), True, True, False),
}
LDS_CASES = list(TABLE)
SOUP = "soup-black"                         # not LDS-resident: the global-scene kernels
TABLE[SOUP] = (None, True, False, True)
CASES = LDS_CASES + [SOUP]
OVERFLOW = [k for k in CASES if not TABLE[k][3]]
FINITE = [k for k in CASES if TABLE[k][3]]

_cache = {}


def rays():
    if "rays" not in _cache:
        o, d = KP.rays(N_RAYS, 3)
        _cache["rays"] = (o[:N_RAYS], d[:N_RAYS])
    return _cache["rays"]


def base(cornell, name):
    """The unedited scene a case is made from: the Cornell box, or for soup-black its 300-triangle soup."""
    if name != SOUP:
        return cornell[2]
    if "soup" not in _cache:
        _cache["soup"] = KP.soup_scene(cornell, 300, 9)
    return _cache["soup"]


def case(cornell, name):
    """The FlatScene of one catalogue entry; `cornell` is the session fixture.  Built once per process and
    not modified by its users.  soup-black is soup_scene(cornell, 300, 9) with the `black` and `n3` edits:
    the soup's triangles come first and share the floor's row, so the Cornell rows keep their numbers."""
    if name not in _cache:
        if name == SOUP:
            _cache[name] = with_normals(with_row(base(cornell, name), BACK, (0, 0, 0)), N3_EVERY, 3)
        else:
            _cache[name] = TABLE[name][0](cornell[2])
    return _cache[name]

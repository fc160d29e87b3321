"""Small scenes for the eight-wide tree of LDS-resident scenes (tests/test_bvh8_collapse.py on the CPU,
tests/test_gpu_lds_bvh8.py and tests/test_gpu_lds_width_hard.py on the GPU): subsets of the Cornell box
that keep its light, chosen by the shape of their trees, a random soup, the largest soup under the light
that is LDS-resident at both widths, and a chain of growing triangles whose eight-wide tree needs more
stack than the pooled kernel has."""
import numpy as np

import hard_scenes as HS

F = np.float32


def subset(flat, n_other):
    """The Cornell light's triangles and the first `n_other` other triangles, as a scene of its own."""
    lt = [int(t) for t in flat.light_tri]
    ids = np.array(lt + [i for i in range(flat.n_tri) if i not in lt][:n_other], np.int64)
    return HS._per_triangle(flat.tri_v[ids], flat.tri_n[ids], flat.tri_mat[ids], flat.mat, [list(range(len(lt)))],
                            flat.direct_rgb)


def five_triangles(flat):
    """3 leaves: one node at either width, every child a leaf."""
    return subset(flat, 3)


def nine_leaves(flat):
    """18 triangles in 9 leaves: one more than an eight-wide root holds, so the BVH8 has a second level."""
    return subset(flat, 16)


def soup(n=120, seed=17):
    """(n, 9) random triangles.  The default 120 are twice what an LDS-resident scene holds: a triangle is
    160 B with its shading data, a BVH4 node 896 B and a BVH8 node 1792 B in their eight octant copies,
    against 24 KiB; about 60 triangles fit at either width (soup_scene, SOUP_N)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.normal(0, 0.08, (n, 3, 3))).astype(F).reshape(n, 9)


def _under_the_light(flat, tv):
    """The Cornell light over the triangles `tv` (n, 9) of material 0."""
    lt = [int(t) for t in flat.light_tri]
    tri_v = np.concatenate([flat.tri_v[lt], tv])
    tri_n = np.concatenate([flat.tri_n[lt], HS._unit_normals(tv)])
    tri_mat = np.concatenate([flat.tri_mat[lt], np.zeros(tv.shape[0], np.int32)])
    return HS._per_triangle(tri_v, tri_n, tri_mat, flat.mat, [list(range(len(lt)))], flat.direct_rgb)


SOUP_N = 60          # the largest soup that is LDS-resident at both widths (tests/test_gpu_lds_width_hard.py)
SOUP_STEP = 20       # SOUP_N + SOUP_STEP triangles are LDS-resident at neither


def soup_scene(flat, n=SOUP_N):
    """The Cornell light over soup(n): n + 2 triangles."""
    return _under_the_light(flat, soup(n))


def soup_rays(flat, n, seed):
    """n interior rays of the soup scene's own box, as kernel_parity.rays draws them."""
    from kernel_parity import rays
    v = flat.tri_v.reshape(-1, 3)
    return rays(n, seed, lo=v.min(0).astype(np.float64), hi=v.max(0).astype(np.float64))


CHAIN_MAX_LEAF = 1   # PRT_MAX_LEAF for chain(): one triangle per leaf


def chain(flat, n=40):
    """The Cornell light over `n` triangles that grow by 1.5^(1/2) each, three sizes apart: the SAH peels
    them off one by one, and the wide trees are chains of full nodes (eight-wide: more than 32 stack
    entries, four-wide: fewer)."""
    s = 1.5 ** (0.5 * np.arange(n))
    z = np.zeros(n)
    tv = np.stack([3 * s, z, z, 4 * s, z, z, 3 * s, s, z], axis=1).astype(F)
    return _under_the_light(flat, tv)

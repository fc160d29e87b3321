"""The hostile scenes of tests/hard_scenes.py against the oracle alone (no GPU): the inputs contain
what they are built for, so tests/test_gpu_hard_hits.py cannot pass vacuously, and the oracle's two
hit backends agree on all of them.

Each count is a floor below the value measured with the brute-force backend (quoted beside it).
"""
import numpy as np
import pytest

import hard_scenes as HS
from hard_scenes import T_MAX, T_MIN
from oracle import oracle as O


def _closest_ids(osc, o, d, tmin=T_MIN, tmax=T_MAX, backend=O.BACKEND_BRUTE):
    hit, t, tri, _ = osc.closest(o, d, tmin, tmax, backend=backend)
    return np.where(hit != 0, tri, -1).astype(np.int64), t


@pytest.mark.parametrize("name", HS.CASES)
def test_scene_is_valid(cornell, name):
    """What prt_scene_create checks (validate_scene), and unit normals, restated in NumPy."""
    flat, sets = HS.case(cornell, name)
    n = flat.n_tri
    assert flat.tri_v.shape == (n, 9) and flat.tri_n.shape == (n, 3) and np.isfinite(flat.tri_v).all()
    assert np.abs(np.linalg.norm(flat.tri_n.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert flat.tri_mat.min() >= 0 and flat.tri_mat.max() < flat.mat.shape[0]
    assert flat.n_light >= 1 and flat.light_off[0] == 0 and (np.diff(flat.light_off) >= 1).all()
    assert flat.light_off[-1] == flat.light_tri.shape[0]
    assert flat.light_tri.min() >= 0 and flat.light_tri.max() < n
    assert (flat.mat[flat.tri_mat[flat.light_tri], 3] > 0).all()            # lights emit
    assert n <= 450
    for o, d in sets.values():
        assert o.shape == d.shape and o.shape[0] <= 20000 and np.isfinite(o).all() and np.isfinite(d).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_lattice_ties_are_exact_and_resolved_to_the_lowest_id(axis):
    flat, rays = HS.lattice(axis)
    osc = O.OracleScene.from_flat(flat)
    for k, (o, d, expect, cand) in enumerate(rays):
        oid, t = _closest_ids(osc, o, d)
        assert np.array_equal(oid, expect), (axis, k)
        h = oid >= 0
        assert h.sum() >= 240                                   # 289, 289, 255, 240
        assert np.unique(t[h]).size == 1, (axis, k, np.unique(t[h]))
        assert (cand >= 2).sum() >= 200, (cand >= 2).sum()      # measured 255, 255, 232, 224
        assert (cand >= 6).sum() >= 40, (cand >= 6).sum()       # measured 49: the interior cell corners
        # open interval: a bound equal to t misses, one ulp inside hits, for t_max and for t_min
        tt = t[h]
        assert (_closest_ids(osc, o[h], d[h], T_MIN, tt)[0] == -1).all()
        assert np.array_equal(_closest_ids(osc, o[h], d[h], T_MIN, np.nextafter(tt, np.float32(np.inf)))[0], oid[h])
        assert (_closest_ids(osc, o[h], d[h], tt, T_MAX)[0] == -1).all()
        assert np.array_equal(_closest_ids(osc, o[h], d[h], np.nextafter(tt, np.float32(0)), T_MAX)[0], oid[h])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_small_lattice_ties_decide_the_radiance(axis):
    """lattice_small, the lattice of the LDS-resident kernels (tests/test_gpu_lds_width_hard.py): at least
    half its rays end on a bit-equal tie (the reference gives 0.65), the brute-force winner is the float64
    expectation, and for at least 0.3 of the paths (the reference alone gives 0.48) the oracle's radiance at
    depth 4 changes when the triangle order, and with it every tie's winner, is reversed: a kernel that
    resolves ties otherwise cannot produce the oracle's image.  Conditions on the input, not measurements."""
    flat, (o, d, expect, cand) = HS.lattice_small(axis)
    n = flat.n_tri
    assert n == 34 and o.shape == d.shape == (HS.N_LATTICE_SMALL_RAYS, 3) and flat.n_light == 1
    assert set(flat.tri_mat[:32]) == {0, 1, 2} and (flat.mat[flat.tri_mat[flat.light_tri], 3] > 0).all()
    assert np.abs(np.linalg.norm(flat.tri_n.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.unique(flat.mat[:3, :3], axis=0).shape[0] == 3
    osc = O.OracleScene.from_flat(flat)
    oid, _ = _closest_ids(osc, o, d)
    assert np.array_equal(oid, expect)
    ties = HS.tie_rays(flat, o, d)
    assert not (ties & (cand < 2)).any()
    assert ties.mean() >= 0.5, ties.mean()
    L = osc.trace_rays(o, d, 4, seed=17)
    R = O.OracleScene.from_flat(HS.reindexed(flat, np.arange(n)[::-1])).trace_rays(o, d, 4, seed=17)
    assert np.isfinite(L).all() and np.isfinite(R).all() and L.mean() > 0
    changed = np.any(L.view(np.uint32) != R.view(np.uint32), axis=1)
    print(f"lattice_small axis {axis}: tie share {ties.mean():.3f}, radiance changed on {changed.mean():.3f}")
    assert changed.mean() >= 0.3, changed.mean()


def test_cornell_far_rays_hit_and_tie(cornell, oracle_scene):
    flat, sets = HS.case(cornell, "cornell")
    assert HS.tie_rays(flat, *sets["interior"]).sum() >= 40      # measured 94: box bottoms coplanar with the floor
    for e in HS.FAR_EXTENTS:
        o, d = sets["far%d" % e]
        centre, extent = HS.scene_box(flat)
        dist = np.linalg.norm(o.astype(np.float64) - centre, axis=1) / extent
        assert dist.min() > 0.99 * e - 0.5 and dist.max() < 1.01 * e + 0.5
        oid, t = _closest_ids(oracle_scene, o, d)
        assert (oid >= 0).mean() >= 0.9                          # measured 1.0
        assert t[oid >= 0].max() < T_MAX
        assert HS.tie_rays(flat, o, d).sum() >= 100, e           # measured 329 and 265


def test_far_distance_is_capped_below_t_max(cornell):
    """A scene scaled by 2^10 would get no hit at all from 100 extents away (204 800 > t_max)."""
    flat, sets = HS.case(cornell, "box-p1")
    _, extent = HS.scene_box(flat)
    assert 100 * extent > T_MAX
    assert HS.far_rays(flat, 16, 0, 100.0)[2] == 0.4 * float(T_MAX)
    osc = O.OracleScene.from_flat(flat)
    for e in HS.FAR_EXTENTS:
        assert (_closest_ids(osc, *sets["far%d" % e])[0] >= 0).mean() >= 0.9


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_layers_tie_on_the_coincident_floor(cornell, seed):
    flat, sets = HS.case(cornell, "layers-%d" % seed)
    assert flat.n_tri == 36 + 10 + 20 and flat.n_light == 2
    floor = cornell[2].tri_v[0:2]
    copies = [np.nonzero((flat.tri_v == q).all(axis=1))[0] for q in floor]
    assert all(c.size == 6 for c in copies)
    assert len({int(flat.tri_mat[i]) for i in copies[0]}) >= 4                      # different materials
    ties = HS.tie_rays(flat, *sets["interior"])
    assert ties.sum() >= 1000, ties.sum()                                            # measured 1971
    # the winner on the floor is the lowest-index copy, whichever material the shuffle gave it
    oid, _ = _closest_ids(O.OracleScene.from_flat(flat), *sets["interior"])
    on_floor = np.isin(oid, np.concatenate(copies))
    assert on_floor.sum() >= 1000 and set(oid[on_floor]) <= {int(c.min()) for c in copies}


def test_layers_seeds_put_different_copies_first(cornell):
    firsts = set()
    for s in range(3):
        flat = HS.case(cornell, "layers-%d" % s)[0]
        k = np.nonzero((flat.tri_v == cornell[2].tri_v[0]).all(axis=1))[0].min()
        firsts.add(int(flat.tri_mat[k]))
    assert len(firsts) >= 2, firsts


@pytest.mark.parametrize("name,nn,ne", [("slivers-1e-3", 32, 8), ("slivers-1e-5", 32, 8), ("slivers8-1e-5", 8, 2)])
def test_slivers_are_hit_when_aimed_at(cornell, name, nn, ne):
    flat, sets = HS.case(cornell, name)
    assert flat.n_tri == 36 + nn + 3 * ne + 1
    v = flat.tri_v.reshape(-1, 3, 3).astype(np.float64)
    area2 = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    flatones, tiny = slice(nn, nn + 2 * ne), slice(nn + 2 * ne, nn + 3 * ne)     # points and collinear; extent 1e-6
    assert (area2[flatones] == 0).all() and (area2[:nn] > 0).all() and (area2[tiny] > 0).all()
    assert np.array_equal(flat.tri_n[flatones], np.tile(np.float32([0, 1, 0]), (2 * ne, 1)))
    assert (np.ptp(v[tiny], axis=1).max(axis=1) <= 1.1e-6).all()
    o, d = sets["aimed+random"]
    oid, _ = _closest_ids(O.OracleScene.from_flat(flat), o, d)
    on_needle = (oid[:4096] >= 0) & (oid[:4096] < nn)
    assert on_needle.sum() >= 2500, on_needle.sum()                 # measured 3128, 3081 and 3011
    assert np.unique(oid[:4096][on_needle]).size == nn              # every needle is hit


@pytest.fixture(scope="module")
def bvh_of(cornell):
    """name -> (oracle scene with the library's BVH2 attached, the Bvh)."""
    from pyrenderer_amd._native import Bvh
    made = {}

    def get(name):
        if name not in made:
            flat = HS.case(cornell, name)[0]
            b = Bvh(flat.tri_v)                                   # max_leaf 4, as prt_scene_create
            nodes, tris, order = b.export()
            assert np.bincount(order, minlength=flat.n_tri).min() >= 1
            osc = O.OracleScene.from_flat(flat)
            osc.set_bvh(nodes, order)
            made[name] = (osc, b, order)
        return made[name]
    return get


def test_some_triangle_is_referenced_from_several_leaves(bvh_of):
    """With the triangle larger than the box in the scene, the builder's spatial splits give the large
    triangles (the walls among them) several references each: one id can be reached through several
    leaves, at equal t, and must still be reported once."""
    for name in ("slivers-1e-3", "slivers-1e-5", "slivers8-1e-5"):
        _, b, order = bvh_of(name)
        refs = np.bincount(order)
        assert refs.max() >= 2 and (refs >= 2).sum() >= 4, refs            # measured: up to 4 references
        assert b.n_tri == order.shape[0] > refs.shape[0]


def test_coincident_copies_land_in_different_leaves(bvh_of, cornell):
    for s in range(3):
        _, b, order = bvh_of("layers-%d" % s)
        assert b.n_leaves >= 66 // 4 and b.depth >= 5


@pytest.mark.parametrize("name", HS.CASES)
def test_oracle_bvh_backend_equals_brute_force(cornell, bvh_of, name):
    """BACKEND_BVH walks the library's exported BVH2 and is the checker of config 4 and of bench.py's
    CPU leg: its boxes may only prune.  Hit, t and id equal the brute-force backend's on every ray
    set.  Before hit_all_bvh put the gamma factor on `best` as well, the far ray sets failed here:
    28 and 30 of 20 000 rays on the plain box, up to 10 of 6000 on its 2^-10 placements."""
    osc, _, _ = bvh_of(name)
    for key, (o, d) in HS.case(cornell, name)[1].items():
        bid, bt = _closest_ids(osc, o, d)
        vid, vt = _closest_ids(osc, o, d, backend=O.BACKEND_BVH)
        bad = np.nonzero((bid != vid) | ((bid >= 0) & (bt != vt)))[0]
        assert bad.size == 0, (name, key, bad.size, [(o[i], d[i], bid[i], vid[i], bt[i], vt[i]) for i in bad[:3]])
        # bounded any-hit queries: the same boolean
        tmax = HS.random_bounds(osc, o, d, 3)
        hb = osc.closest(o, d, T_MIN, tmax)[0]
        hv = osc.closest(o, d, T_MIN, tmax, backend=O.BACKEND_BVH)[0]
        assert np.array_equal(hb, hv), (name, key)

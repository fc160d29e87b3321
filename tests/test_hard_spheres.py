"""The hostile sphere scenes of tests/hard_spheres.py against the oracle alone (no GPU): the inputs
contain what they are built for, so tests/test_gpu_hard_spheres.py cannot pass vacuously, and the
oracle's sphere rules are what include/prt.h states: the interval is closed at both ends, a sphere at
the triangles' t wins, the highest index wins among equal sphere roots, a NaN t_max is accepted.

Each count is a floor below the value measured with the brute-force backend (quoted beside it).
"""
import numpy as np
import pytest

import hard_spheres as S
from kernel_parity import T_MAX, T_MIN, nee_mode, random_bounds
from oracle import oracle as O

F = np.float32
UP, DOWN = F(np.inf), F(0)


def _osc(cornell, name):
    return O.OracleScene.from_flat(S.case(cornell, name)[0])


def _closest_ids(osc, o, d, tmin=T_MIN, tmax=T_MAX, backend=O.BACKEND_BRUTE):
    hit, t, tri, _ = osc.closest(o, d, tmin, tmax, backend=backend)
    return np.where(hit != 0, tri, -1).astype(np.int64), t


def _sphere_ids(flat, oid):
    """Sphere index of each hit id, -1 for triangles and misses."""
    return np.where(oid >= flat.n_tri, oid - flat.n_tri, -1)


@pytest.mark.parametrize("name", S.CASES)
def test_scene_is_valid_and_its_radiance_finite(cornell, name):
    """What prt_scene_create checks, restated; every path of every ray set ends finite at depth 8
    under both direct-lighting estimators, and the sets carry light."""
    flat, sets = S.case(cornell, name)
    n_sph = flat.sph.shape[0]
    assert flat.sph.shape == (n_sph, 4) and flat.sph_mat.shape == (n_sph,) and n_sph >= 1
    assert np.isfinite(flat.sph).all() and (flat.sph[:, 3] > 0).all()
    assert flat.sph_mat.min() >= 0 and flat.sph_mat.max() < flat.mat.shape[0]
    assert flat.tri_mat.max() < flat.mat.shape[0] and np.isfinite(flat.mat).all()
    assert (flat.mat[flat.tri_mat[flat.light_tri], 3] > 0).all() and flat.n_light >= 1
    assert ((flat.mat[:, :3] >= 2.0 ** -40) & (flat.mat[:, :3] <= 2.0 ** 40)).all()     # shade_fast stays on
    osc = O.OracleScene.from_flat(flat)
    for key, (o, d) in sets.items():
        assert o.shape == d.shape and o.shape[0] <= 4096 and np.isfinite(o).all() and np.isfinite(d).all()
        for mis in (False, True):
            with nee_mode(mis):
                L = osc.trace_rays(o, d, 8, seed=17)
            assert np.isfinite(L).all() and L.mean() > 0, (name, key, mis)


def test_zoo_holds_every_row_and_arrangement(cornell):
    flat, _ = S.case(cornell, "zoo")
    rows = flat.mat[flat.sph_mat]
    assert {1.5, 2.4, 1.0, 0.75} <= set(rows[rows[:, 5] == 3][:, 6].astype(np.float64).round(6))
    metal = rows[rows[:, 5] == 2]
    assert (metal[:, 7] == 0).any() and (metal[:, 7] > 1).any()
    lam = rows[(rows[:, 5] == 0) & (rows[:, 3] == 0)]
    assert (lam[:, 4] == 0).any() and (lam[:, 4] != 0).any()
    assert (rows[:, 3] != 0).any()                                      # an emitter row that no light list names
    c, r = flat.sph[:, :3].astype(np.float64), flat.sph[:, 3].astype(np.float64)
    dist = np.linalg.norm(c[:, None] - c[None], axis=2)
    a, b = S.ZOO_COINCIDENT
    assert np.array_equal(flat.sph[a], flat.sph[b]) and flat.sph_mat[a] != flat.sph_mat[b]
    assert abs(dist[4, 5] - (r[4] + r[5])) < 1e-6                       # the tangent pair
    assert dist[0, 1] + r[1] < r[0] and dist[6, 7] == 0 and abs(r[6] - r[7] - 0.01) < 1e-6
    v = flat.tri_v.reshape(-1, 3).astype(np.float64)
    assert (np.linalg.norm(v - c[8], axis=1) < r[8]).all()              # the box lies inside sphere 8
    assert c[9, 1] == r[9] and r[S.ZOO_SMALL] == F(1e-3)                # tangent to the floor y = 0


def test_zoo_interior_rays_reach_every_sphere(cornell):
    flat, sets = S.case(cornell, "zoo")
    oid, _ = _closest_ids(_osc(cornell, "zoo"), *sets["interior"])
    sid = _sphere_ids(flat, oid)
    assert (sid >= 0).mean() >= 0.20, (sid >= 0).mean()                  # measured 0.262
    per = np.bincount(sid[sid >= 0], minlength=flat.sph.shape[0])
    print("zoo interior: share on spheres %.3f, per sphere %s" % ((sid >= 0).mean(), per))
    assert per[S.ZOO_COINCIDENT[0]] == 0                                 # the lower index of the pair never wins
    others = np.delete(per, [S.ZOO_COINCIDENT[0], S.ZOO_SMALL])
    assert others.min() >= 10, per          # measured 108 15 0 69 30 31 101 50 503 32 0 29 64 41


def test_zoo_inside_rays_leave_through_their_own_sphere(cornell):
    flat, sets = S.case(cornell, "zoo")
    o, d = sets["inside"]
    n_sph = flat.sph.shape[0]
    own = np.arange(o.shape[0]) % n_sph
    c, r = flat.sph[:, :3].astype(np.float64), flat.sph[:, 3].astype(np.float64)
    assert (np.linalg.norm(o.astype(np.float64) - c[own], axis=1) < r[own]).all()
    oid, t = _closest_ids(_osc(cornell, "zoo"), o, d)
    sid = _sphere_ids(flat, oid)
    within = np.linalg.norm(c[:, None] - c[None], axis=2) + r[None, :] <= r[:, None]    # [k, j]: j lies in k
    ok = (sid >= 0) & within[own, np.maximum(sid, 0)]
    print("zoo inside: first hit on the own sphere or one in it %.3f" % ok.mean())
    assert ok.mean() >= 0.90, ok.mean()                                  # measured 0.996
    # total internal reflection at the first vertex of the rays that start in an IOR-2.4 sphere and hit it
    # from inside, restated in float64: ratio = ior (back side), sin(theta) * ratio > 1
    sel = np.isin(own, S.ZOO_IOR24) & (sid == own)
    p = o[sel].astype(np.float64) + d[sel].astype(np.float64) * t[sel, None]
    cos = np.einsum("ij,ij->i", d[sel].astype(np.float64), (p - c[own[sel]]) / r[own[sel], None])
    tir = 2.4 * np.sqrt(np.maximum(0.0, 1 - cos * cos)) > 1
    print("zoo inside: %d of %d rays from inside an IOR-2.4 sphere reflect totally" % (tir.sum(), sel.sum()))
    assert sel.sum() >= 200 and tir.sum() >= sel.sum() / 4, (tir.sum(), sel.sum())   # measured 225 of 293


# ------------------------------------------------------------------ dyadic: the answer by hand
def _mt64(flat, o, d):
    """Moeller-Trumbore of the reference in float64 over all triangles: (lowest id of the closest, t)."""
    v = flat.tri_v.reshape(-1, 3, 3).astype(np.float64)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    best_t, best_id = np.full(o.shape[0], np.inf), np.full(o.shape[0], -1)
    for i in range(v.shape[0]):
        c = np.cross(e1[i], d)
        det = c @ e2[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / det
            s = o - v[i, 0]
            q = np.cross(s, e2[i])
            t = -f * (q @ e1[i])
            u = -f * np.einsum("ij,ij->i", q, d)
            w = f * np.einsum("ij,ij->i", c, s)
            hit = (np.abs(det) > 0) & (float(T_MIN) < t) & (t < best_t) & (0 <= u) & (u <= 1) & (w >= 0) & (1 - u - w >= 0)
        best_t, best_id = np.where(hit, t, best_t), np.where(hit, i, best_id)
    return best_id, best_t


def _expected_dyadic(flat, o, d, meta):
    """(id, t, exact) per axis ray, in float64.  A sphere of centre c and radius r meets the ray at
    `along` -+ sqrt(r^2 - u^2 - v^2), `along` the distance to the centre plane and (u, v) the offsets in
    it; all of these are exact, the square root is rounded to f32 once, as is the root.  The near root
    counts if it lies in [t_min, best], else the far one; the spheres follow the triangles in index order,
    so a sphere at the triangles' t takes the hit and so does a later sphere at an earlier one's t."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    tid, tt = _mt64(flat, o, d)
    eid, et = tid.copy(), np.where(tid >= 0, tt, float(T_MAX))
    axis, sign = meta[:, 1], meta[:, 2]
    rows = np.arange(o.shape[0])
    for k, (c, r, _) in enumerate(S.DYADIC):
        rel = np.array(c) - o
        along = rel[rows, axis] * sign
        perp2 = (rel ** 2).sum(1) - rel[rows, axis] ** 2
        h2 = r * r - perp2
        sq = np.sqrt(np.maximum(h2, 0)).astype(F).astype(np.float64)
        near, far = ((along + s * sq).astype(F).astype(np.float64) for s in (-1, 1))
        root = np.where((near >= float(T_MIN)) & (near <= et), near, far)
        take = (h2 >= 0) & (root >= float(T_MIN)) & (root <= et)
        eid, et = np.where(take, flat.n_tri + k, eid), np.where(take, root, et)
    # t is exactly representable for spheres and for the axis-aligned walls (materials 0 .. 4)
    exact = (eid >= flat.n_tri) | ((eid >= 0) & (flat.tri_mat[np.maximum(np.minimum(eid, flat.n_tri - 1), 0)] <= 4))
    return eid, et.astype(F), exact


def test_dyadic_hits_ties_and_normals_are_exact(cornell):
    flat, _ = S.case(cornell, "dyadic")
    osc = _osc(cornell, "dyadic")
    n_tri = flat.n_tri
    for kind, (o, d, meta) in S.dyadic_rays().items():
        oid, t = _closest_ids(osc, o, d)
        eid, et, exact = _expected_dyadic(flat, o, d, meta)
        # the 68 rays that run inside the floor plane y = 0 graze the boxes' bottom faces (y = -1.1e-16): float64
        # and f32 decide those edge-on triangles differently, so the expectation by hand leaves them out
        off = (o[:, 1] != 0) | (d[:, 1] != 0)
        assert (~off).sum() == 68
        assert np.array_equal(oid[off], eid[off]), (kind, np.nonzero(off & (oid != eid))[0][:5])
        exact &= off
        assert np.array_equal(t[exact], et[exact]) and exact.sum() >= 2800, kind    # measured 2909 / 3091 of 3468
        on_axis = (meta[:, 3] == 8) & (meta[:, 4] == 8)
        mine = on_axis if kind == "centre" else on_axis & (oid >= n_tri)   # from outside a box can stand in between
        assert mine.sum() >= 10 and (oid[mine] == n_tri + meta[mine, 0]).all()
        assert (oid != n_tri).all() and (oid == n_tri + 1).sum() >= 900  # measured 985 / 1158
        # the poles: rays along +-y on the sphere's axis
        pole = on_axis & (meta[:, 1] == 1)
        rec = osc.hit_all(o[pole], d[pole], T_MIN, T_MAX, seed=5)
        want_y = -d[pole, 1]                  # two-sided Lambert rows: the normal faces the ray
        assert pole.sum() == 4 and np.array_equal(rec[:, 6], want_y), (kind, rec[:, 5:8])
        assert not rec[:, 5].any() and not rec[:, 7].any()
        if kind == "centre":                  # leaving through the bottom / the top: t = r exactly
            assert np.array_equal(rec[:, 1], F([0.25] * 4))
            # the ray from the centre of the floor-tangent pair straight down ties with the floor
            tie = pole & (meta[:, 0] == 1) & (meta[:, 2] == -1)
            assert tie.sum() == 1 and _mt64(flat, o[tie].astype(np.float64), d[tie].astype(np.float64))[1][0] == 0.25
            assert oid[tie][0] == n_tri + 1 and t[tie][0] == F(0.25)
            low = np.nonzero(pole & (meta[:, 2] == 1))[0]              # straight up: flipped, (-0, -1, -0)
            assert np.array_equal(osc.closest(o[low], d[low], T_MIN, T_MAX)[3].view(np.uint32),
                                  np.tile(F([-0.0, -1.0, -0.0]).view(np.uint32), (2, 1)))


@pytest.mark.parametrize("name,key", [("zoo", "interior"), ("zoo", "inside"), ("dyadic", "above"), ("dyadic", "centre")])
def test_sphere_interval_is_closed_at_both_ends(cornell, name, key):
    """t_max == root and t_min == root still hit the sphere; one ulp inside the root they do not."""
    flat, sets = S.case(cornell, name)
    osc = _osc(cornell, name)
    o, d = sets[key]
    oid, t = _closest_ids(osc, o, d)
    h = oid >= flat.n_tri
    assert h.sum() >= 1000
    o, d, oid, t = o[h], d[h], oid[h], t[h]
    hid, ht = _closest_ids(osc, o, d, T_MIN, t)
    assert np.array_equal(hid, oid) and np.array_equal(ht, t)
    assert (_closest_ids(osc, o, d, T_MIN, np.nextafter(t, DOWN))[0] == -1).all()
    assert (osc.closest(o, d, T_MIN, t)[0] != 0).all()
    lid, lt = _closest_ids(osc, o, d, t, T_MAX)
    assert np.array_equal(lid, oid) and np.array_equal(lt, t)
    nid, nt = _closest_ids(osc, o, d, np.nextafter(t, UP), T_MAX)
    assert ((nid != oid) | (nt > t)).all()


def nan_bound_expectation(flat, o, d):
    """Rays that meet a sphere at some root >= t_min, in float64 (rays closer than 1e-9 of a decision
    are left out: the third array)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    meets, sure = np.zeros(o.shape[0], bool), np.ones(o.shape[0], bool)
    for c in flat.sph.astype(np.float64):
        oc = o - c[:3]
        a, hb = (d * d).sum(1), (oc * d).sum(1)
        disc = hb * hb - a * ((oc * oc).sum(1) - c[3] * c[3])
        far = (-hb + np.sqrt(np.maximum(disc, 0))) / a
        meets |= (disc >= 0) & (far >= float(T_MIN))
        sure &= (np.abs(disc) > 1e-9) & (np.abs(far - float(T_MIN)) > 1e-9)
    return meets, sure


def test_nan_bound_hits_spheres_only(cornell):
    """t_max = NaN (the reference's shadow bound when p2.x == p.x): no triangle is accepted, every sphere
    the ray meets is."""
    nan = F(np.nan)
    flat, sets = S.case(cornell, "dyadic")
    osc = _osc(cornell, "dyadic")
    for key, (o, d) in sets.items():
        hit = osc.closest(o, d, T_MIN, nan)[0] != 0
        meets, sure = nan_bound_expectation(flat, o, d)
        assert np.array_equal(hit[sure], meets[sure]) and sure.mean() > 0.9
        only_tri = (_closest_ids(osc, o, d)[0] >= 0) & ~meets & sure
        print("dyadic %s under a NaN bound: %d rays hit a sphere, %d meet only triangles" % (key, hit.sum(), only_tri.sum()))
        assert hit.sum() >= 1000 and only_tri.sum() >= 500 and not hit[only_tri].any()   # measured 2364 / 1018 and 2316 / 986
    flat, sets = S.case(cornell, "zoo")
    assert (_osc(cornell, "zoo").closest(*sets["interior"], T_MIN, nan)[0] != 0).all()   # sphere 8 surrounds them


@pytest.mark.parametrize("k", range(len(S.SPECKS)))
def test_speck_normals_are_far_from_unit(cornell, k):
    """The f32 normal (p - c) / r of a small sphere, with p = o + d t rounded as the kernels round it:
    most hits have a length outside [0.5, 2], up to 108 (r = 1e-3 from 200 away), 8658 (r = 1e-4 from 2000
    away) and 9.9 (r = 1e-4 from 2 away)."""
    name = S.speck_name(*S.SPECKS[k])
    flat, sets = S.case(cornell, name)
    o, d = sets["aimed"]
    oid, t = _closest_ids(_osc(cornell, name), o, d)
    h = oid == flat.n_tri
    p = o[h] + d[h] * t[h, None]                                          # f32, ray.at
    ln = np.linalg.norm(((p - flat.sph[0, :3]) / flat.sph[0, 3]).astype(np.float64), axis=1)
    out = (ln < 0.5) | (ln > 2)
    print("%s: %d sphere hits, %d normals outside [0.5, 2], lengths %.4g .. %.4g" % (name, h.sum(), out.sum(), ln.min(), ln.max()))
    assert h.sum() >= 2000, h.sum()                                       # measured 3276, 3009, 3081
    assert out.sum() >= 1000, out.sum()                                   # measured 2200, 1558, 2072
    assert ln.max() > (100 if k < 2 else 5), ln.max()                     # measured 108, 8658, 9.86


def test_many_spheres_are_hit(cornell):
    flat, sets = S.case(cornell, "many")
    assert flat.sph.shape[0] == S.N_MANY
    sid = _sphere_ids(flat, _closest_ids(_osc(cornell, "many"), *sets["interior"])[0])
    assert np.unique(sid[sid >= 0]).size >= 60 and (sid >= 0).mean() >= 0.1, np.unique(sid).size   # measured 67, 0.155
    assert len(set(flat.sph_mat)) == len(S.ROW_NAMES)


@pytest.mark.parametrize("name", ["soup-zoo", "zoo", "many"])
def test_oracle_bvh_backend_equals_brute_force(cornell, name):
    """BACKEND_BVH on the library's BVH2 with the spheres after it, as tests/test_hard_scenes.py has it for
    triangles: hit, t and id equal the brute-force backend's, and so does every bounded any-hit boolean."""
    from pyrenderer_amd._native import Bvh
    flat, sets = S.case(cornell, name)
    nodes, _, order = Bvh(flat.tri_v).export()
    osc = O.OracleScene.from_flat(flat)
    osc.set_bvh(nodes, order)
    for key, (o, d) in sets.items():
        bid, bt = _closest_ids(osc, o, d)
        vid, vt = _closest_ids(osc, o, d, backend=O.BACKEND_BVH)
        bad = np.nonzero((bid != vid) | ((bid >= 0) & (bt != vt)))[0]
        assert bad.size == 0, (name, key, bad.size, [(o[i], d[i], bid[i], vid[i], bt[i], vt[i]) for i in bad[:3]])
        tmax = random_bounds(osc, o, d, 3)
        hb = osc.closest(o, d, T_MIN, tmax)[0]
        assert np.array_equal(hb, osc.closest(o, d, T_MIN, tmax, backend=O.BACKEND_BVH)[0]), (name, key)
        assert 0.2 < (hb != 0).mean() < 0.8

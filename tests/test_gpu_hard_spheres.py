"""Hit and path parity on hostile spheres and specular materials (tests/hard_spheres.py): many spheres
(nested, coincident, tangent, a shell, one around the box and the camera, one of r = 1e-3), every
material row on a sphere, dyadic spheres whose ties and axis normals are exact, and specks whose f32
normal (p - c) / r has a length between 0.006 and 8658.

Everything is compared bit for bit with the oracle's brute-force backend, so there is no tolerance
anywhere.  The hit level goes through `prt_closest_hits` (f32 and quantised nodes) and pins the sphere
rules of include/prt.h: the interval closed at both ends, a sphere at the triangles' t wins, the highest
index wins among equal roots, a NaN bound is accepted.  `prt_hit_all` pins the device's to_world (its
two special branches on the dyadic poles) in all 16 floats; `prt_trace_rays` runs every trace-kernel
variant; `prt_render_tiles` the pooled kernel's own copy of the sphere loop and the counters;
`prt_features` the first-hit features on sphere pixels.

All inputs are finite and valid; tests/test_hard_spheres.py shows with the oracle alone that they
contain the hits, ties, total reflections and non-unit normals they are built for.
"""
import numpy as np
import pytest

import hard_spheres as S
from kernel_parity import (ALL_VARIANTS, T_MAX, T_MIN, OracleRefs, check_trace, hits_wrong, is_mis, packed_camera,
                           random_bounds, variant_flags, world_cache, wrong_rows)

pytestmark = pytest.mark.gpu

F = np.float32
UP, DOWN, NAN = F(np.inf), F(0), F(np.nan)
SPECK0 = S.speck_name(*S.SPECKS[0])
REFS = OracleRefs()


@pytest.fixture(scope="module")
def world(cornell):
    """name -> (DeviceScene, OracleScene, ray sets); each scene is created once for the module."""
    yield from world_cache(lambda name: S.case(cornell, name))


def _closest_wrong(ds, osc, o, d, tmin, tmax, quantized):
    return hits_wrong(ds, osc, o, d, tmin, tmax, quantized, any_hit=False)[:2]


def _any_wrong(ds, osc, o, d, tmin, tmax, quantized):
    return hits_wrong(ds, osc, o, d, tmin, tmax, quantized, any_hit=True)


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name", S.CASES)
def test_hits_match_brute_force(world, name, quantized):
    """Closest hit in (id, t) and bounded any-hit as a boolean, on every ray set of the scene; the
    message names every ray set that differs, with its first rays and both answers."""
    ds, osc, sets = world(name)
    wrong = []
    for key, (o, d) in sets.items():
        n, first = _closest_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized)
        if n:
            wrong.append((key, "closest", n, first))
        n, first, ohit = _any_wrong(ds, osc, o, d, T_MIN, random_bounds(osc, o, d, 3), quantized)
        if n:
            wrong.append((key, "any-hit", n, first))
        assert 0.2 < ohit.mean() < 0.8                           # the bounds do separate the rays
    assert not wrong, (name, [w[:3] for w in wrong], wrong)


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name,key", [("zoo", "interior"), ("zoo", "inside"), ("dyadic", "above"), ("dyadic", "centre")])
def test_sphere_interval_is_closed_and_nan_bound_accepted(world, name, key, quantized):
    """On the rays that end on a sphere: t_max == root and t_min == root still hit it (closest and
    any-hit), one ulp inside the root they do not.  On all rays: under t_max = NaN exactly the oracle's
    rays hit, which are those that meet a sphere (tests/test_hard_spheres.py)."""
    ds, osc, sets = world(name)
    o, d = sets[key]
    flat = ds.flat
    hit, t, tri, _ = osc.closest(o, d, T_MIN, T_MAX)
    h = (hit != 0) & (tri >= flat.n_tri)
    assert h.sum() >= 1000
    so, sd, st, sid = o[h], d[h], t[h], tri[h]
    for any_hit in (False, True):
        def q(tmin, tmax):
            return ds.closest_hits(so, sd, tmin, tmax, any_hit=any_hit, quantized=quantized)
        for gid, gt in (q(T_MIN, st), q(st, T_MAX)):               # closed at the upper and at the lower end
            if any_hit:
                assert (gid >= 0).all(), (any_hit, np.nonzero(gid < 0)[0][:5])
            else:
                assert np.array_equal(gid, sid) and np.array_equal(gt, st), np.nonzero((gid != sid) | (gt != st))[0][:5]
        assert (q(T_MIN, np.nextafter(st, DOWN))[0] == -1).all(), any_hit
        if not any_hit:
            gid, gt = q(np.nextafter(st, UP), T_MAX)
            assert ((gid != sid) | (gt > st)).all()
    for tmin, tmax in ((T_MIN, st), (st, T_MAX), (T_MIN, np.nextafter(st, DOWN)), (np.nextafter(st, UP), T_MAX)):
        n, first = _closest_wrong(ds, osc, so, sd, tmin, tmax, quantized)
        assert n == 0, (n, first)
        n, first, _ = _any_wrong(ds, osc, so, sd, tmin, tmax, quantized)
        assert n == 0, (n, first)
    n, first = _closest_wrong(ds, osc, o, d, T_MIN, NAN, quantized)
    assert n == 0, (n, first)
    n, first, ohit = _any_wrong(ds, osc, o, d, T_MIN, NAN, quantized)
    assert n == 0, (n, first)
    assert ohit.any() and (name == "zoo" or not ohit.all())        # zoo: sphere 8 surrounds every ray


@pytest.mark.parametrize("quantized", [False, True])
def test_dyadic_ties_go_to_the_sphere_and_to_the_higher_index(world, quantized):
    """The ray from the centre of the floor-tangent pair straight down ends at t = 0.25 on the floor and on
    both spheres: the sphere wins over the triangle and the higher index over the lower; no ray of the
    grids ever ends on the lower one."""
    ds, _, _ = world("dyadic")
    n_tri = ds.flat.n_tri
    rays = S.dyadic_rays()
    o, d, meta = rays["centre"]
    tie = np.nonzero((meta[:, 0] == 1) & (meta[:, 1] == 1) & (meta[:, 2] == -1) & (meta[:, 3] == 8) & (meta[:, 4] == 8))[0]
    assert tie.size == 1 and np.array_equal(o[tie[0]], F([0.5, 0.25, -0.5])) and np.array_equal(d[tie[0]], F([0, -1, 0]))
    gid, gt = ds.closest_hits(o, d, T_MIN, T_MAX, quantized=quantized)
    assert gid[tie[0]] == n_tri + 1 and gt[tie[0]] == F(0.25), (gid[tie[0]], gt[tie[0]])
    own = (meta[:, 3] == 8) & (meta[:, 4] == 8)                    # from a centre along every axis: t = r
    assert np.array_equal(gid[own], n_tri + meta[own, 0]) and (gt[own] == F(0.25)).all()
    # the triangles alone end that ray on the floor at the same t
    fid, ft = ds.closest_hits(o[tie], d[tie], T_MIN, np.nextafter(F(0.25), UP), quantized=quantized)
    assert fid[0] == n_tri + 1 and ft[0] == F(0.25)
    for key in rays:
        gid, _ = ds.closest_hits(*rays[key][:2], T_MIN, T_MAX, quantized=quantized)
        assert (gid != n_tri).all() and (gid == n_tri + 1).sum() >= 900


# ------------------------------------------------------------------ prt_hit_all
@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name", ["zoo", "dyadic", SPECK0])
def test_hit_all_records_match_the_oracle(world, name, quantized):
    """All 16 floats of World.hit_all's record per ray as bits: hit, t, p, the flipped normal, the emissive
    flag, the attenuation, the scattered direction and its pdf, which run to_world on the device for every
    sphere hit (on the dyadic poles its v.y == 1 and v.y == -1 branches)."""
    ds, osc, sets = world(name)
    for key, (o, d) in sets.items():
        want = osc.hit_all(o, d, T_MIN, T_MAX, seed=11)
        got = ds.hit_all(o, d, T_MIN, T_MAX, seed=11, quantized=quantized)
        bad = wrong_rows(got, want)
        assert bad.size == 0, (name, key, bad.size, [(i, o[i], d[i], got[i], want[i]) for i in bad[:3]])
        assert (want[:, 0] != 0).mean() > 0.8
    if name == "dyadic":
        for key, (o, d, meta) in S.dyadic_rays().items():
            pole = (meta[:, 3] == 8) & (meta[:, 4] == 8) & (meta[:, 1] == 1)
            got = ds.hit_all(o[pole], d[pole], T_MIN, T_MAX, seed=11, quantized=quantized)
            assert pole.sum() == 4 and np.array_equal(got[:, 6], -d[pole, 1]) and not got[:, 5].any() and not got[:, 7].any()
            assert (got[:, 15] > 0).all()                       # a Lambert row: scattered through to_world


# ------------------------------------------------------------------ kernel level
N_TRACE, DEPTH = 4096, 8
TRACE_CASES = {"zoo": ("zoo", "interior"), "zoo-inside": ("zoo", "inside"), "dyadic-above": ("dyadic", "above"),
               "dyadic-centre": ("dyadic", "centre"), "many": ("many", "interior")}
TRACE_CASES.update({S.speck_name(r, dist): (S.speck_name(r, dist), "aimed") for r, dist in S.SPECKS})


def _check_trace(ds, osc, case, o, d, v, lds_scene=True):
    ref = REFS.trace(case, osc, o, d, DEPTH, 17, is_mis(v))
    check_trace(ds, ref, o, d, DEPTH, 17, v, label=case, lds_scene=lds_scene)


@pytest.mark.parametrize("v", ALL_VARIANTS)
@pytest.mark.parametrize("case", list(TRACE_CASES))
def test_every_kernel_variant_traces_the_oracles_paths(world, case, v):
    """Up to 4096 caller rays, depth 8, through each forced trace-kernel variant (the reference estimator's
    and both MIS ones): every path's radiance equals the oracle's, bit for bit.  The specks put normals of
    length 0.006 .. 8658 through lambert_div and nee_div under shade_fast."""
    name, key = TRACE_CASES[case]
    ds, osc, sets = world(name)
    o, d = sets[key]
    _check_trace(ds, osc, case, o[:N_TRACE], d[:N_TRACE], v)


def test_an_lds_resident_sphere_scene_takes_all_eight_variants(world):
    """Spheres stay in global memory, so the zoo (the Cornell box's triangles) is LDS-resident and every
    variant id names a kernel that exists for it: the parametrised test above runs eight different ones."""
    from pyrenderer_amd import _native as N
    ds, _, _ = world("zoo")
    assert sorted(ALL_VARIANTS) == sorted(list(N.VAR_REFERENCE) + list(N.VAR_MIS)) == list(range(1, N.VAR_LAST + 1))
    ran = {ds.kernel_info(n_items=N_TRACE, flags=variant_flags(v))["variant"] for v in ALL_VARIANTS}
    assert ran == set(range(1, 9)) and ds.kernel_info()["lds_scene"]


@pytest.mark.parametrize("key", ["interior", "inside"])
@pytest.mark.parametrize("v", [3, 5])
def test_global_kernels_trace_the_soup_zoo(world, v, key):
    """The zoo's spheres in a 300-triangle soup, which is not LDS-resident: the global-scene kernels
    (quantised nodes, suspended tails), reference and MIS."""
    ds, osc, sets = world("soup-zoo")
    o, d = sets[key]
    _check_trace(ds, osc, "soup-zoo-" + key, o[:N_TRACE], d[:N_TRACE], v, lds_scene=False)


# ------------------------------------------------------------------ render level
@pytest.mark.parametrize("kernel", ["default", "lds"])
def test_zoo_render_and_counters_match_the_oracle(world, cornell, kernel):
    """32 x 32, 4 spp, depth 8 through prt_render_tiles: camera rays that start inside the IOR-1 sphere,
    the pooled kernel's own sphere loop (the default for this scene) and the phase-aligned kernel, bit for
    bit; the extension and shadow query counts equal the oracle's and no sample is non-finite."""
    from pyrenderer_amd import _native as N
    ds, osc, _ = world("zoo")
    cam = packed_camera(cornell)
    ids = np.arange(1, dtype=np.int32)
    flags = N.PRT_FLAG_STATS | ((N.VAR_LDS << 8) if kernel == "lds" else 0)
    want_var = N.VAR_LDS if kernel == "lds" else N.VAR_LDS_POOL
    assert ds.kernel_info(n_items=32 * 32 * 4, flags=flags)["variant"] == want_var
    ref, oc = REFS.render_tiles("zoo", osc, cam, 32, 32, 32, ids, 4, 8, 9)
    assert np.isfinite(ref).all() and ref.mean() > 0
    for fl in (flags, flags & ~N.PRT_FLAG_STATS):
        got, st = ds.render_tiles(cam, 32, 32, 32, 32, ids, 4, 8, 9, fl)
        np.testing.assert_array_equal(got, ref)
        if fl & N.PRT_FLAG_STATS:
            assert (st[2], st[3]) == oc and st[0] > 0 and st[1] > 0, (st, oc)
            assert ds.diag_stats()[N.PRT_DIAG_NONFINITE] == 0


# ------------------------------------------------------------------ features
def test_zoo_features_on_sphere_pixels(world, cornell):
    """prt_features on the zoo at 48 x 48, 2 samples, against the host composition (prt_camera_rays,
    prt_hit_all, float32 sums), bit for bit; primary rays do end on Lambert spheres."""
    from pyrenderer_amd.denoise import features_packed_host
    ds, osc, _ = world("zoo")
    flat = ds.flat
    pc = packed_camera(cornell)
    W = H = 48
    o, d, _ = ds.camera_rays(pc, W, H, 16, 16, np.arange(9, dtype=np.int32), 0, 2, 7)
    hit, _, tri, _ = osc.closest(o, d, T_MIN, T_MAX)
    row = flat.mat[flat.sph_mat[np.maximum(tri - flat.n_tri, 0)]]
    lambert = (hit != 0) & (tri >= flat.n_tri) & (row[:, 5] == 0) & (row[:, 3] == 0)
    assert lambert.sum() >= 50, lambert.sum()
    got = ds.features(pc, W, H, samples=2, seed=7)
    want = features_packed_host(ds, pc, W, H, samples=2, seed=7, tile=16)
    diff = np.argwhere(np.any(got.view(np.uint32) != want.view(np.uint32), axis=-1))
    assert len(diff) == 0, (len(diff), diff[:5])
    assert (got[..., 7] > 0).all()                                  # sphere 8 surrounds the camera: no miss
    ds.check_faults()

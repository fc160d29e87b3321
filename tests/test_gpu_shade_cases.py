"""The guarded side of the shading quotients, and the boundary of the cheap side, on the GPU
(tests/shade_cases.py): Cornell boxes with a black wall, a pure red one, albedo channels of 1e-20, 1e-40
and one ulp below 2^-40, a light with zero channels, face normals of length 3, 0.25 and just above 2, an
albedo of 2^41 whose throughput overflows (TraceParams::shade_fast off: div3_nan_guard / div3 with the
reference's pdf = 1e-4 rule inside the LDS kernels), and albedos of exactly 2^-40 and 2^40, normals of
length exactly 2 and 0.5 (shade_fast on: lambert_div / nee_div at the edge of their proven domain).

Everything is compared bit for bit with the oracle's brute-force backend, so there is no tolerance
anywhere.  Where a throughput overflows the oracle's radiance holds infinities and NaNs: there the NaN
masks must be equal and every other float, the infinities included, bit-equal; host and device may
disagree on a NaN's payload and on nothing else.  `kernel_info()` pins that each scene really runs the
side it claims; `prt_trace_rays` runs every trace-kernel variant; `prt_render_tiles` the pooled and the
phase-aligned kernel from camera rays with their counters; `prt_hit_all` the non-unit normals' record;
`prt_features` and the denoiser an albedo of exactly 0.

What these tests can tell apart, tried once on an MI355X: with div3_nan_guard's plain divisions replaced
by a multiplication with v_rcp_f32 (one ulp off), 56 of them fail: every variant on black, red, tiny,
denormal, below and above, variants 3 and 5 on lo-edge and on the soup, and all four renders.  With the
shade_fast test taken out of lambert_div and nee_div all of them still pass: the flag bounds what is
proven, and on these inputs the shared-reciprocal sequence happens to round as the division does.

tests/test_shade_cases.py shows with the host's classification and the oracle alone that the inputs
contain what they are built for.
"""
import numpy as np
import pytest

import shade_cases as C
from kernel_parity import (ALL_VARIANTS, T_MAX, T_MIN, OracleRefs, check_trace, is_mis, packed_camera, variant_flags,
                           world_cache, wrong_rows)

pytestmark = pytest.mark.gpu

F = np.float32
REFS = OracleRefs()


@pytest.fixture(scope="module")
def world(cornell):
    """name -> (DeviceScene, OracleScene); each scene is created once for the module."""
    yield from world_cache(lambda name: (C.case(cornell, name),))


@pytest.mark.parametrize("name", C.CASES)
def test_the_live_scene_reports_the_tables_flags(world, name):
    """kernel_info()'s shade_fast and plain are the uploaded scene's own: what the table says, for a large
    launch and for every forced variant alike, so the tests below run the side they claim."""
    ds, _ = world(name)
    _, plain, shade_fast, _ = C.TABLE[name]
    info = ds.kernel_info()
    assert (info["plain"], info["shade_fast"]) == (plain, shade_fast), (name, info)
    assert info["lds_scene"] == (name != C.SOUP), (name, info)
    for v in ALL_VARIANTS:
        i = ds.kernel_info(n_items=C.N_RAYS, flags=variant_flags(v))
        assert (i["plain"], i["shade_fast"]) == (plain, shade_fast), (name, v, i)


def test_the_unedited_box_reports_both_flags_set(gpu_scene):
    info = gpu_scene.kernel_info()
    assert info["plain"] and info["shade_fast"] and info["lds_scene"], info


# ------------------------------------------------------------------ kernel level
def _check_trace(ds, osc, name, v, lds_scene=True):
    o, d = C.rays()
    ref = REFS.trace(name, osc, o, d, C.DEPTH, C.SEED, is_mis(v))
    check_trace(ds, ref, o, d, C.DEPTH, C.SEED, v, label=name, lds_scene=lds_scene,
                expect={"shade_fast": C.TABLE[name][2]}, finite=C.TABLE[name][3])


@pytest.mark.parametrize("v", ALL_VARIANTS)
@pytest.mark.parametrize("name", C.LDS_CASES)
def test_every_kernel_variant_traces_the_oracles_paths(world, name, v):
    """4096 caller rays, depth 8, seed 17 through each forced trace-kernel variant (the reference
    estimator's and both MIS ones): every path's radiance equals the oracle's bit for bit; on `above` and
    `hi-edge`, whose throughput overflows (3 non-finite rows under the reference estimator, 76 under MIS,
    6 of them with a NaN), NaN for NaN and bit for bit elsewhere."""
    ds, osc = world(name)
    _check_trace(ds, osc, name, v)


def test_an_lds_case_takes_all_eight_variants(world):
    from pyrenderer_amd import _native as N
    ds, _ = world("black")
    assert sorted(ALL_VARIANTS) == sorted(list(N.VAR_REFERENCE) + list(N.VAR_MIS)) == list(range(1, N.VAR_LAST + 1))
    ran = {ds.kernel_info(n_items=C.N_RAYS, flags=variant_flags(v))["variant"] for v in ALL_VARIANTS}
    assert ran == set(range(1, 9))


@pytest.mark.parametrize("v", [3, 5])
def test_global_kernels_trace_the_black_soup(world, v):
    """The black wall and the normals of length 3 in a 300-triangle soup, which is not LDS-resident: the
    global-scene kernels' div3_nan_guard and div3, reference and MIS."""
    ds, osc = world(C.SOUP)
    _check_trace(ds, osc, C.SOUP, v, lds_scene=False)


# ------------------------------------------------------------------ render level
SEED_ABOVE = 6       # chosen with the oracle alone: 2 of the 1024 pixels overflow (seeds 1, 3, 5, 7 give 1; 2, 4, 8 none)


@pytest.mark.parametrize("kernel", ["default", "lds"])
@pytest.mark.parametrize("name", ["black", "above"])
def test_render_and_counters_match_the_oracle(world, cornell, name, kernel):
    """32 x 32, depth 8 through prt_render_tiles, with PRT_FLAG_STATS and without, in the pooled kernel (the
    default for these scenes) and the phase-aligned one.  `black` at 4 spp: the image bit for bit, the
    extension and shadow query counts, no non-finite sample.  `above` at 1 spp, where a pixel's sum is its
    sample: the image NaN for NaN and bit for bit elsewhere, and the non-finite counter equals the number of
    non-finite oracle pixels."""
    from pyrenderer_amd import _native as N
    ds, osc = world(name)
    cam = packed_camera(cornell)
    ids = np.arange(1, dtype=np.int32)
    spp, seed = (4, 9) if name == "black" else (1, SEED_ABOVE)
    flags = N.PRT_FLAG_STATS | ((N.VAR_LDS << 8) if kernel == "lds" else 0)
    want_var = N.VAR_LDS if kernel == "lds" else N.VAR_LDS_POOL
    info = ds.kernel_info(n_items=32 * 32 * spp, flags=flags)
    assert info["variant"] == want_var and not info["shade_fast"], info
    ref, oc = REFS.render_tiles(name, osc, cam, 32, 32, 32, ids, spp, 8, seed)
    bad_ref = int((~np.isfinite(ref)).any(axis=1).sum())
    assert (bad_ref == 0 and ref.mean() > 0) if name == "black" else bad_ref >= 1, bad_ref
    for fl in (flags, flags & ~N.PRT_FLAG_STATS):
        got, st = ds.render_tiles(cam, 32, 32, 32, 32, ids, spp, 8, seed, fl)
        bad = wrong_rows(got, ref, nan_aware=name == "above")
        assert bad.size == 0, (name, kernel, fl, bad.size, [(i, got[i], ref[i]) for i in bad[:3]])
        if fl & N.PRT_FLAG_STATS:
            assert (st[2], st[3]) == oc and st[0] > 0 and st[1] > 0, (st, oc)
            assert ds.diag_stats()[N.PRT_DIAG_NONFINITE] == bad_ref, (ds.diag_stats()[N.PRT_DIAG_NONFINITE], bad_ref)


# ------------------------------------------------------------------ prt_hit_all
@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name", ["n3", "n-quarter"])
def test_hit_all_records_carry_the_non_unit_normal(world, name, quantized):
    """All 16 floats of World.hit_all's record per ray as bits: the non-unit normal in [5:8], the direction
    scattered through the normalised frame and pdf = |n . wi| / pi with the non-unit n."""
    ds, osc = world(name)
    o, d = C.rays()
    want = osc.hit_all(o, d, T_MIN, T_MAX, seed=11)
    got = ds.hit_all(o, d, T_MIN, T_MAX, seed=11, quantized=quantized)
    bad = wrong_rows(got, want)
    assert bad.size == 0, (name, quantized, bad.size, [(i, o[i], d[i], got[i], want[i]) for i in bad[:3]])
    ln = np.linalg.norm(want[:, 5:8].astype(np.float64), axis=1)
    scale = 3 if name == "n3" else 0.25
    scaled = (want[:, 0] != 0) & (np.abs(ln - scale) < 1e-5)
    assert scaled.sum() >= 500 and ((want[:, 0] != 0) & (np.abs(ln - 1) < 1e-5)).sum() >= 500, scaled.sum()
    lam = scaled & (want[:, 8] == 0)                                    # not the light: a scattered direction
    wi = want[lam, 12:15].astype(np.float64)
    assert lam.sum() >= 400 and np.abs(np.linalg.norm(wi, axis=1) - 1).max() < 1e-5
    cos = np.einsum("ij,ij->i", want[lam, 5:8].astype(np.float64), wi)
    assert np.abs(want[lam, 15] - np.abs(cos) / np.pi).max() < 1e-5 * scale


# ------------------------------------------------------------------ features and the denoiser
def test_black_wall_features_and_denoised_frame(world, cornell):
    """prt_features on `black` at 48 x 48, 2 samples, against the host composition bit for bit; the albedo
    is exactly 0 on the pixels whose samples all end on the black wall, and the filter, which divides the
    colour by the albedo, leaves a 4-spp render of the scene finite everywhere."""
    from pyrenderer_amd.denoise import denoise, features_packed_host
    from pyrenderer_amd.device_scene import unpack_tiles
    ds, _ = world("black")
    pc = packed_camera(cornell)
    W = H = 48
    got = ds.features(pc, W, H, samples=2, seed=7)
    want = features_packed_host(ds, pc, W, H, samples=2, seed=7, tile=16)
    diff = np.argwhere(np.any(got.view(np.uint32) != want.view(np.uint32), axis=-1))
    assert len(diff) == 0, (len(diff), diff[:5])
    black = (want[..., 7] == 1) & ~want[..., 0:3].any(axis=-1)          # every sample hit, albedo sum exactly 0
    assert black.sum() >= 100, black.sum()
    assert not got[black][:, 0:3].view(np.uint32).any()                 # +0.0 in all three channels
    ds.check_faults()
    ids = np.arange(9, dtype=np.int32)
    sums, _ = ds.render_tiles(pc, W, H, 16, 16, ids, 4, 8, 9, 0)
    mean = unpack_tiles(sums, W, H, 16, 16, ids) / F(4)
    assert np.isfinite(mean).all() and mean.mean() > 0
    out = denoise(mean, got)
    assert out.shape == (W, H, 3) and np.isfinite(out).all() and out.mean() > 0

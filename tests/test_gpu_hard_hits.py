"""Hit and path parity on hostile geometry (tests/hard_scenes.py): exact ties, coincident quads,
needles and degenerate triangles, a triangle referenced from several leaves, scenes placed far from
the origin and at other scales, and rays from 100 and 1000 scene extents away.

Everything is compared bit for bit with the oracle's brute-force backend, the plain restatement of
the same f32 arithmetic, so there is no tolerance anywhere: the closest hit must be the brute-force
(t, lowest id) whatever the visiting order, and no box may cull a hit.  The hit level goes through
`prt_closest_hits` (f32 and quantised nodes); the kernel level through `prt_trace_rays` with every
trace-kernel variant forced (LDS octant copies, 16-bit stacks, the pooled kernel's suspended tails,
the global kernel's spill stack), which had only seen the Cornell box's own placement before.

All inputs are finite and valid; tests/test_hard_scenes.py shows with the oracle alone that they
contain the ties, needle hits and far hits they are built for.
"""
import numpy as np
import pytest

import hard_scenes as HS
from kernel_parity import (ALL_VARIANTS, T_MAX, T_MIN, OracleRefs, check_trace, hits_wrong, is_mis, packed_camera,
                           random_bounds, world_cache)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

UP, DOWN = np.float32(np.inf), np.float32(0)
REFS = OracleRefs()


@pytest.fixture(scope="module")
def world(cornell):
    """name -> (DeviceScene, OracleScene, ray sets); each scene is created once for the module."""
    yield from world_cache(lambda name: HS.case(cornell, name))


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name", HS.CASES)
def test_hits_match_brute_force(world, name, quantized):
    """Closest hit in (id, t) and bounded any-hit as a boolean, on every ray set of the scene; the
    message names every ray set that differs, with its first rays and both answers."""
    ds, osc, sets = world(name)
    wrong = []
    for key, (o, d) in sets.items():
        want = REFS.closest((name, key), osc, o, d)
        n, first, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized, any_hit=False, want=want)
        if n:
            wrong.append((key, "closest", n, first))
        tmax = REFS.get(("bounds", name, key), lambda: random_bounds(osc, o, d, 3))
        n, first, ohit = hits_wrong(ds, osc, o, d, T_MIN, tmax, quantized, any_hit=True)
        if n:
            wrong.append((key, "any-hit", n, first))
        assert 0.2 < ohit.mean() < 0.8                           # the bounds do separate the rays
    assert not wrong, (name, [w[:3] for w in wrong], wrong)


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_lattice_ties_and_open_bounds(world, axis, quantized):
    """Exact ties on up to six triangles go to the lowest id (the float64 expectation), and the
    interval is open at both ends: a bound equal to t misses, one ulp inside hits."""
    ds, osc, _ = world("lattice-" + HS.AXES[axis])
    for o, d, expect, _ in HS.lattice(axis)[1]:
        gid, gt = ds.closest_hits(o, d, T_MIN, T_MAX, quantized=quantized)
        assert np.array_equal(gid, expect), np.nonzero(gid != expect)[0][:5]
        h = expect >= 0
        o, d, t, want = o[h], d[h], gt[h], expect[h]
        assert np.unique(t).size == 1
        for any_hit in (True, False):
            def ids(tmin, tmax):
                return ds.closest_hits(o, d, tmin, tmax, any_hit=any_hit, quantized=quantized)[0]
            assert (ids(T_MIN, t) == -1).all(), any_hit
            assert (ids(t, T_MAX) == -1).all(), any_hit
            inside_hi, inside_lo = ids(T_MIN, np.nextafter(t, UP)), ids(np.nextafter(t, DOWN), T_MAX)
            if any_hit:
                assert (inside_hi >= 0).all() and (inside_lo >= 0).all()
            else:
                assert np.array_equal(inside_hi, want) and np.array_equal(inside_lo, want)


# ------------------------------------------------------------------ kernel level
N_TRACE, DEPTH = 4096, 4
# the 93 triangles of slivers(1e-5) are more than the LDS-resident kernels hold (24 KiB of scene): they see the
# same mixture with 8 needles (51 triangles); the full scene goes through the global-scene kernels below
TRACE_CASES = {"layers": ("layers-0", "interior"), "slivers": ("slivers8-1e-5", "aimed+random"),
               "far100": ("cornell", "far100"), "far1000": ("cornell", "far1000"),
               "translated": ("box-p2", "interior"), "scaled-down": ("box-p0", "interior")}


def _variant_ids():
    from pyrenderer_amd import _native as N
    return list(N.VAR_REFERENCE) + list(N.VAR_MIS)


def _check_trace(ds, osc, case, o, d, v, lds_scene=True):
    ref = REFS.trace(case, osc, o, d, DEPTH, 17, is_mis(v))
    check_trace(ds, ref, o, d, DEPTH, 17, v, label=case, lds_scene=lds_scene)


@pytest.mark.parametrize("v", ALL_VARIANTS)
@pytest.mark.parametrize("case", list(TRACE_CASES))
def test_every_kernel_variant_traces_the_oracles_paths(world, case, v):
    """4096 caller rays, depth 4, through each forced trace-kernel variant (the reference
    estimator's and both MIS ones): every path's radiance equals the oracle's, bit for bit."""
    assert sorted(_variant_ids()) == [1, 2, 3, 4, 5, 6, 7, 8]
    name, key = TRACE_CASES[case]
    ds, osc, sets = world(name)
    o, d = sets[key]
    _check_trace(ds, osc, case, o[:N_TRACE], d[:N_TRACE], v)


@pytest.mark.parametrize("case", list(TRACE_CASES))
def test_spill_stack_traces_the_oracles_paths(cornell, case, monkeypatch):
    """The global-scene kernel with a 4-entry LDS stack (PRT_SPILL_LDS=4, read at scene creation):
    the deeper entries of these trees go through the global spill area."""
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.device_scene import DeviceScene
    name, key = TRACE_CASES[case]
    flat, sets = HS.case(cornell, name)
    monkeypatch.setenv("PRT_SPILL_LDS", "4")
    ds = DeviceScene(flat, 0)
    try:
        assert ds.kernel_info(n_items=N_TRACE, flags=N.VAR_GLOBAL << 8)["stack"] == 4
        need = ds.kernel_info(n_items=N_TRACE, flags=N.VAR_LDS_POOL << 8)["stack"]   # the BVH4's exact bound
        assert need > 5, need
        o, d = sets[key]
        _check_trace(ds, O.OracleScene.from_flat(flat), case, o[:N_TRACE], d[:N_TRACE], N.VAR_GLOBAL)
    finally:
        ds.close()


@pytest.mark.parametrize("v", [3, 5])
def test_global_kernels_trace_the_full_sliver_scene(world, v):
    """slivers(1e-5) whole (32 needles, 93 triangles, 113 references) is not LDS-resident: its aimed
    rays through the global-scene kernels (quantised nodes, suspended tails), reference and MIS."""
    ds, osc, sets = world("slivers-1e-5")
    o, d = sets["aimed+random"]
    _check_trace(ds, osc, "slivers-full", o[:N_TRACE], d[:N_TRACE], v, lds_scene=False)


# ------------------------------------------------------------------ stack bound
@pytest.mark.parametrize("name", ["layers-0", "layers-1", "layers-2", "slivers8-1e-5"])
def test_stack_depth_within_the_collapse_bound(world, cornell, name):
    """Coincident geometry forces object-median splits and a deeper tree; the large triangle adds
    references.  As tests/test_gpu_stack.py does for the Cornell scenes: the deepest stack entry a
    render touches (diag word 13) stays within the bound the kernel's stack was sized to."""
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.device_scene import interleaved_tiles
    ds, _, _ = world(name)
    packed = packed_camera(cornell)
    W = H = 64
    tiles = interleaved_tiles(W, H, 64)
    for var in N.VAR_POOL + (N.VAR_LDS,):
        flags = N.PRT_FLAG_STATS | (var << 8)
        info = ds.kernel_info(n_items=W * H * 4, flags=flags)
        assert info["variant"] == var
        ds.render_tiles(packed, W, H, 64, 64, tiles, 4, 8, seed=1, flags=flags)
        deepest = int(ds.diag_stats()[N.PRT_DIAG_MAX_STACK])
        assert 1 <= deepest <= info["stack"], (name, var, deepest, info)

"""Hostile geometry through both tree widths of the LDS trace kernels.  The width rule (prt_plan.cpp
lds_width) gives the two-level hostile scenes (layers-*, slivers8-*) the BVH4 and every Cornell-sized one
the BVH8, so with PRT_LDS_WIDTH unset visit_node8 / copy_octant_nodes8 never see coincident quads,
needles, degenerate triangles, duplicated references, a second level of inner nodes or more than 15 stack
entries, and the width-4 instantiations never see far rays, other placements or spheres.  Here every case
runs at both forced widths (env PRT_LDS_WIDTH, read at scene creation) through each LDS reference variant
(1, 2, 6: phase-aligned; 7, 8: pooled), and each test first asserts the width, the variant and the LDS
residency that the launch reports, so that it cannot pass on another kernel.

Everything is compared bit for bit with the oracle's brute-force backend; there is no tolerance anywhere.
tests/test_hard_scenes.py and tests/test_hard_spheres.py show with the oracle alone that the inputs contain
what they are built for, tests/test_bvh8_collapse.py that the trees are the shapes relied on here.
"""
import numpy as np
import pytest

import bvh8_scenes as S8
import hard_scenes as HS
import hard_spheres as SP
from kernel_parity import OracleRefs, all_tiles, check_trace, packed_camera, render_twice
from kernel_parity import scenes_by_width as scenes  # noqa: F401  (the module-scoped fixture)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_TRACE, DEPTH = 4096, 4                # as tests/test_gpu_hard_hits.py traces the same scenes
WIDTHS = (4, 8)
REFS = OracleRefs()
LDS_VARIANTS = (1, 2, 6, 7, 8)          # the variants that take the width (prt_plan.h variant_takes_width)
CORNELL_NEED8 = 15                      # the Cornell BVH8's stack bound: the deepest a benign scene asks for
SPECK0 = SP.speck_name(*SP.SPECKS[0])


def _hard(name, key):
    return lambda cornell: (HS.case(cornell, name)[0],) + tuple(HS.case(cornell, name)[1][key])


def _sphere(name, key):
    return lambda cornell: (SP.case(cornell, name)[0],) + tuple(SP.case(cornell, name)[1][key])


def _slivers8(cornell):
    """2048 rays aimed at the needles, then 2048 random interior ones."""
    flat, sets = HS.case(cornell, "slivers8-1e-5")
    o, d = sets["aimed+random"]
    pick = np.r_[0:N_TRACE // 2, 4096:4096 + N_TRACE // 2]
    return flat, o[pick], d[pick]


_tie_rays = {}     # case -> mask of the rays that end on more than one triangle (lattice cases)


def _lattice_small(axis):
    def make(cornell):
        flat, (o, d, _, cand) = HS.lattice_small(axis)
        _tie_rays["lattice-small-" + HS.AXES[axis]] = cand[:N_TRACE] >= 2
        return flat, o, d
    return make


def _soup(cornell):
    flat = S8.soup_scene(cornell[2], S8.SOUP_N)
    return (flat,) + S8.soup_rays(flat, N_TRACE, 71)


# case -> (scene name of the cache, builder of (flat, o, d)); the rays are cut to N_TRACE
TRACE_CASES = {
    "layers-0": ("layers-0", _hard("layers-0", "interior")),
    "layers-1": ("layers-1", _hard("layers-1", "interior")),
    "slivers8": ("slivers8-1e-5", _slivers8),
    "cornell-far100": ("cornell", _hard("cornell", "far100")),
    "cornell-far1000": ("cornell", _hard("cornell", "far1000")),
    "box-p2": ("box-p2", _hard("box-p2", "interior")),
    "box-p0": ("box-p0", _hard("box-p0", "interior")),
    "box-p3": ("box-p3", _hard("box-p3", "interior")),
    "box-p2-axis": ("box-p2", _hard("box-p2", "axis")),
    "lattice-small-x": ("lattice-small-x", _lattice_small(0)),
    "lattice-small-y": ("lattice-small-y", _lattice_small(1)),
    "lattice-small-z": ("lattice-small-z", _lattice_small(2)),
    "soup": ("soup", _soup),
    "zoo": ("zoo", _sphere("zoo", "interior")),
    "zoo-inside": ("zoo", _sphere("zoo", "inside")),
    "dyadic-above": ("dyadic", _sphere("dyadic", "above")),
    "many": ("many", _sphere("many", "interior")),
    SPECK0: (SPECK0, _sphere(SPECK0, "aimed")),
}
# the scenes of six or seven BVH8 nodes, which the default rule leaves at width 4; the others have three
DEFAULT_4 = ("layers-0", "layers-1", "slivers8-1e-5", "soup")
_built = {}


def _case(cornell, case):
    """(scene name, flat, o, d, OracleScene) of one case, built once."""
    if case not in _built:
        name, make = TRACE_CASES[case]
        flat, o, d = make(cornell)
        _built[case] = (name, flat, o[:N_TRACE], d[:N_TRACE], O.OracleScene.from_flat(flat))
    return _built[case]


# ------------------------------------------------------------------ 4a: path level
def test_the_cases_are_the_ones_the_width_rule_moved(scenes, cornell):
    """With PRT_LDS_WIDTH unset the two-level hostile scenes run at width 4 and the Cornell-sized cases at
    width 8: the halves of the cross product below that no other test reaches.  Forced, every case takes
    either width."""
    for case in TRACE_CASES:
        name, flat, _, _, _ = _case(cornell, case)
        info = scenes(name, flat, None).kernel_info()
        assert info["lds_scene"], (case, info)
        assert info["bvh_arity"] == (4 if name in DEFAULT_4 else 8), (case, info)
        for width in WIDTHS:
            assert scenes(name, flat, width).kernel_info()["bvh_arity"] == width, (case, width)


@pytest.mark.parametrize("v", LDS_VARIANTS)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("case", list(TRACE_CASES))
def test_hostile_paths_at_both_widths(scenes, cornell, case, width, v):
    """Up to 4096 caller rays, depth 4, seed 17 through prt_trace_rays: every path's radiance bits equal the
    oracle's, at either tree width, in each LDS reference variant."""
    name, flat, o, d, osc = _case(cornell, case)
    check_trace(scenes(name, flat, width), REFS.trace(case, osc, o, d, DEPTH, 17, False), o, d, DEPTH, 17, v,
                label="%s at width %d" % (case, width), lds_scene=True, width=width, ties=_tie_rays.get(case))


# ------------------------------------------------------------------ 4b: render level
RENDER_KERNELS = {"default": 0, "lds": 1, "pool": 7}     # name -> forced variant id (0: the scene's default)


def _render_case(cornell, name):
    """(flat, camera, oracle image, oracle counters) of one 64 x 64 render, computed once."""
    def compute():
        flat = S8.soup_scene(cornell[2], S8.SOUP_N) if name == "soup" else HS.case(cornell, name)[0]
        cam = packed_camera(cornell)
        osc = O.OracleScene.from_flat(flat)
        ref, counted = REFS.render_tiles(name, osc, cam, 64, 64, 64, all_tiles(64, 64, 64), 4, 8, 11)
        assert np.isfinite(ref).all() and ref.mean() > 0
        return flat, cam, ref, counted
    return REFS.get(("case", name), compute)


@pytest.mark.parametrize("kernel", list(RENDER_KERNELS))
@pytest.mark.parametrize("name", ["layers-0", "slivers8-1e-5", "soup"])
def test_hostile_renders_at_both_widths(scenes, cornell, name, kernel):
    """64 x 64, 4 spp, depth 8, one tile through prt_render_tiles, by the scene's default variant, by the
    phase-aligned kernel and by the pooled kernel (these scenes' pooled layout does not fit seven blocks per
    CU, so their default is the phase-aligned kernel without an occupancy target and the pooled one has to be
    asked for): the width-8 image equals the width-4 image and the oracle's, the STATS image the production
    one, the extension and shadow query counts the oracle's counters; no non-finite sample, no watchdog
    trip, and the deepest stack entry touched stays within the bound the stack was sized to (render_twice asserts
    the last four).

    The deepest stack at width 8 is printed.  It is not deeper than the Cornell BVH8's bound of 15 entries:
    the first run gave 10 on layers-0, 7 on slivers8-1e-5 and 5 on the soup with each of the three kernels
    (9, 8 and 5 at width 4), under bounds of 22, 22 and 15.  Bvh8Host::stack_need is the worst case of a ray
    that hits every child of every node on its way, which no ray of these renders does, so there is no
    such assertion here; that the two-level trees ask for more than 15 entries is asserted on the CPU
    (tests/test_bvh8_collapse.py) and on the stack the launch reports, and the inputs are not bent to reach
    the bound on the GPU."""
    from pyrenderer_amd import _native as N
    flat, cam, ref, counted = _render_case(cornell, name)
    variant = RENDER_KERNELS[kernel]
    ids = all_tiles(64, 64, 64)
    got = {}
    for width in WIDTHS:
        ds = scenes(name, flat, width)
        assert ds.kernel_info()["lds_scene"]
        got[width] = render_twice(ds, cam, 64, 64, 64, ids, 4, 8, 11, variant << 8, width=width)
        info = got[width]["info"]
        assert info["variant"] in LDS_VARIANTS
        deepest = int(got[width]["words"][N.PRT_DIAG_MAX_STACK])
        print(f"{name} {kernel}: width {info['bvh_arity']} variant {info['variant']}, deepest stack {deepest} of "
              f"{info['stack']}, {int((got[width]['img'] != ref).any(axis=-1).sum())} pixels differ from the oracle")
        if width == 8 and name != "soup":
            assert info["stack"] > CORNELL_NEED8, info      # sized for more than the Cornell tree ever needs
    assert np.array_equal(got[8]["img"], got[4]["img"]) and np.array_equal(got[8]["img"], ref), name
    assert got[8]["queries"] == got[4]["queries"] == counted, (got[8]["queries"], got[4]["queries"], counted)


# ------------------------------------------------------------------ 4c: suspended tails, two-level BVH8
def test_suspended_tails_on_a_two_level_bvh8(scenes, cornell):
    """PRT_POOL_RESUME_MIN at width 8 on layers-0 (six BVH8 nodes, depth 2), as test_gpu_lds_bvh8's
    test_suspended_tails does on the Cornell box: 1 M items, images and query counts equal across the
    thresholds and equal to the width-4 scene's.  The pooled kernel is forced: it is not this scene's
    default.  No oracle render at this size; the 64 x 64 render above ties the scene to the oracle."""
    from pyrenderer_amd import _native as N
    flat = HS.case(cornell, "layers-0")[0]
    cam = packed_camera(cornell)
    W = H = 256
    ids = all_tiles(W, H, 64)
    pool = N.VAR_LDS_POOL
    got = {thr: render_twice(scenes("layers-0", flat, 8, PRT_POOL_RESUME_MIN=thr), cam, W, H, 64, ids, 16, 8, 2,
                             pool << 8, width=8) for thr in (0, 1, 64)}
    base4 = render_twice(scenes("layers-0", flat, 4, PRT_POOL_RESUME_MIN=0), cam, W, H, 64, ids, 16, 8, 2, pool << 8,
                         width=4)
    suspended = {thr: int(g["words"][N.PRT_DIAG_SUSPENDED]) for thr, g in got.items()}
    print("layers-0 width 8 variant %d, suspensions per threshold:" % pool, suspended)
    assert suspended[0] == 0 and suspended[64] > 0
    for thr in (1, 64):
        assert np.array_equal(got[thr]["img"], got[0]["img"]) and got[thr]["queries"] == got[0]["queries"], thr
    assert np.array_equal(got[0]["img"], base4["img"]) and got[0]["queries"] == base4["queries"]


# ------------------------------------------------------------------ the soup at the LDS limit
def test_soup_size_is_the_largest_at_both_widths(scenes, cornell):
    """SOUP_N triangles under the light are LDS-resident at either forced width (7 BVH8 nodes of 1792 B, 15
    BVH4 nodes of 896 B, 160 B per triangle); SOUP_N + SOUP_STEP are resident at neither.  On the CPU, by
    the formulas of prt_lds_layout.h, no size above SOUP_N fits at both widths."""
    flat = S8.soup_scene(cornell[2], S8.SOUP_N)
    assert S8.SOUP_N == 60 and flat.n_tri == 62
    for width in WIDTHS:
        info = scenes("soup", flat, width).kernel_info()
        assert info["lds_scene"] and info["bvh_arity"] == width, (width, info)
    more = S8.soup_scene(cornell[2], S8.SOUP_N + S8.SOUP_STEP)
    for width in (None, 4, 8):
        info = scenes("soup-more", more, width).kernel_info()
        assert not info["lds_scene"] and info["bvh_arity"] == 4, (width, info)

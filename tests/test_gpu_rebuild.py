"""prt_scene_rebuild on the GPU: a resident scene's trees built again on the device must hold,
word for word, what tests/lbvh_ref.py computes from the vertices alone, and the scene must then answer every
query and render every frame as a freshly created scene and the oracle's brute force do, bit for bit, through
every trace-kernel variant it admits.  Results do not depend on the tree (ties go to the lowest id), so the bound
on every comparison is equality.  What the feature is for is measured too: after a third of a soup moved, the
rebuilt tree is visited strictly less often than the refit one."""
import numpy as np
import pytest

import global_cases as G
import lbvh_ref as L
import refit_ref as R
from kernel_parity import (T_MAX, T_MIN, OracleRefs, all_tiles, check_trace, hits_wrong, is_mis, packed_camera,
                           random_bounds, variant_flags)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LDS_VARIANTS = (1, 2, 6, 7, 8)
GLOBAL_VARIANTS = (3, 5)
W = H = TILE = 64
SPP, DEPTH, SEED = 2, 4, 11
IDS = all_tiles(W, H, TILE)
BVH_ORDER = ("tris", "nodes4", "nodes4q", "nodes8")
ORIGINAL_ORDER = ("tri_nm", "tri_frame", "light_v")
REFS = OracleRefs()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differ(a, b):
    return a.shape != b.shape or int((words(a) != words(b)).sum())


def create(flat, setting=None):
    from pyrenderer_amd.device_scene import DeviceScene
    with G.knobs(setting or {}):
        return DeviceScene(flat, 0)


def with_geometry(flat, tri_v=None, sph=None):
    from pyrenderer_amd.flatten import FlatScene
    return FlatScene(flat.tri_v if tri_v is None else tri_v, flat.tri_n, flat.tri_mat, flat.tri_prim, flat.prim_lo,
                     flat.prim_hi, flat.mat, flat.light_tri, flat.light_off, flat.direct_rgb,
                     flat.sph if sph is None else sph, flat.sph_mat, flat.sph_prim)


def interior(cornell):
    return G.ray_sets(cornell, "soup-3000")["interior"]


def frame_of(ds, cornell, v=0):
    img, _ = ds.render_tiles(packed_camera(cornell), W, H, TILE, TILE, IDS, SPP, DEPTH, SEED, variant_flags(v) if v else 0)
    ds.check_faults()
    return img


def oracle_frame(key, osc, cornell, mis=False):
    return REFS.render_tiles(key, osc, packed_camera(cornell), W, H, TILE, IDS, SPP, DEPTH, SEED, mis=mis)[0]


def check_words(ds, flat, label, lds=True):
    """The downloaded trees against the restatement's; returns the restatement."""
    want = REFS.get(("lbvh", label), lambda: L.rebuild(flat.tri_v, 4, (4, 8) if lds else (4,)))
    if not lds:
        want = dict(want, nodes8=np.zeros((0, 56), np.float32))
    for k in BVH_ORDER:
        got = ds.download(k)
        assert not differ(got, want[k]), (label, k, got.shape, want[k].shape, differ(got, want[k]))
    info = ds.rebuild_info()
    assert (info["nodes4"], info["depth4"], info["need4"]) == (want["nodes4"].shape[0], want["depth4"], want["need4"])
    if lds:
        assert (info["nodes8"], info["depth8"], info["need8"]) == (want["nodes8"].shape[0], want["depth8"], want["need8"])
    assert info["slots"] == flat.n_tri and ds.n_nodes == info["nodes4"] and ds.bvh_depth == info["depth4"]
    assert info["ms"].shape == (8,) and (info["ms"] >= 0).all() and np.isfinite(info["ms"]).all()
    return want


def check_queries(ds, fresh, osc, key, o, d, variants, cornell, width=None, frames=True):
    """Closest hits on f32 and quantised nodes, bounded any-hit, traced paths and a frame of `ds` against brute
    force (and the frame and hits against the fresh scene), each trace and frame through every variant."""
    want = REFS.closest(key, osc, o, d)
    tmax = REFS.get(("bounds", key), lambda: random_bounds(osc, o, d, 5))
    occluded = REFS.get(("any", key), lambda: osc.closest(o, d, T_MIN, tmax)[0] != 0)
    for quantized in (False, True):
        n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized, False, want=want)
        assert n == 0, (key, "closest", quantized, n, bad)
        n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, tmax, quantized, True, want=occluded)
        assert n == 0, (key, "any", quantized, n, bad)
        gid, gt = ds.closest_hits(o, d, T_MIN, T_MAX, quantized=quantized)
        fid, ft = fresh.closest_hits(o, d, T_MIN, T_MAX, quantized=quantized)
        assert np.array_equal(gid, fid) and not differ(gt, ft), (key, quantized)
    for v in variants:
        ref = REFS.trace(key, osc, o, d, DEPTH, SEED, is_mis(v))
        check_trace(ds, ref, o, d, DEPTH, SEED, v, label=f"{key} v{v}", width=width if v in LDS_VARIANTS else None,
                    lds_scene=width is not None, finite=bool(np.isfinite(ref).all()))
        if frames:
            img = frame_of(ds, cornell, v)
            assert not differ(img, oracle_frame(key, osc, cornell, is_mis(v))), (key, v, "frame against the oracle")
            assert not differ(img, frame_of(fresh, cornell, v)), (key, v, "frame against the fresh scene")
    ds.check_faults()


def cornell_moves(cornell):
    """DESIGN.md §13's moves: the short box (primitive 5) spun 6 degrees three times, then the tall box (6)
    carried outside the room."""
    from pyrenderer_amd.scenes import moved, spun
    spins = spun(cornell[0], 5, 6.0, 4)[1:]
    g = np.eye(4)
    g[0, 3] = 3.0
    return [(f"spin-{k + 1}", s) for k, s in enumerate(spins)] + [("tall-out", moved(spins[-1], {6: g}))]


def scattered(flat):
    """A third of the triangles displaced by a tenth of the scene's extent (DESIGN.md §13's degradation pose)."""
    return with_geometry(flat, tri_v=R.displaced(flat.tri_v, extents=0.1))


# ------------------------------------------------------------------ word for word
@pytest.mark.parametrize("name,width", [("cornell", 4), ("cornell", 8), ("soup-3000", 4)])
def test_rebuild_with_the_same_geometry_is_the_restated_tree(cornell, name, width):
    flat = cornell[2] if name == "cornell" else G.scene(cornell, name)
    lds = name == "cornell"
    ds = create(flat, {"PRT_LDS_WIDTH": width})
    try:
        before = {k: ds.download(k) for k in ORIGINAL_ORDER}
        assert ds.rebuild(flat) is ds and ds.last_update == "rebuild"
        check_words(ds, flat, name, lds=lds)
        for k, b in before.items():
            assert not differ(ds.download(k), b), (name, k)
        info = ds.kernel_info()
        assert info["lds_scene"] == lds and (not lds or info["bvh_arity"] == width)
        grown = ds.device_bytes
        assert ds.rebuild(flat).device_bytes == grown         # a second rebuild allocates nothing
        check_words(ds, flat, name, lds=lds)
        ds.check_faults()
    finally:
        ds.close()


# ------------------------------------------------------------------ exact queries
@pytest.mark.parametrize("width", [4, 8])
def test_rebuilt_moved_cornell(cornell, width):
    from pyrenderer_amd.flatten import flatten_scene
    setting = {"PRT_LDS_WIDTH": width}
    o, d = interior(cornell)
    ds = create(cornell[2], setting)
    try:
        for label, scene in cornell_moves(cornell)[2:]:        # the third spin, then the tall box outside
            flat = flatten_scene(scene)
            assert ds.rebuild(flat) is ds and ds.flat is flat
            check_words(ds, flat, label)
            assert ds.kernel_info()["lds_scene"] and ds.kernel_info()["bvh_arity"] == width
            fresh = create(flat, setting)
            try:
                for k in ORIGINAL_ORDER:
                    assert not differ(ds.download(k), fresh.download(k)), (label, k)
                osc = REFS.get(("osc", label), lambda: O.OracleScene.from_flat(flat))
                check_queries(ds, fresh, osc, label, o, d, LDS_VARIANTS + GLOBAL_VARIANTS, cornell, width=width)
            finally:
                fresh.close()
    finally:
        ds.close()


@pytest.mark.parametrize("name", ["soup-3000-scattered", "slivers-1e-5", "soup-zoo"])
def test_rebuilt_global_scenes(cornell, name):
    base = G.scene(cornell, name.replace("-scattered", ""))
    flat = scattered(base) if name.endswith("scattered") else base
    ds = create(base)
    fresh = create(flat)
    try:
        ds.rebuild(flat)
        assert ds.rebuild_info()["need4"] <= 32
        if flat.sph.shape[0]:
            assert not differ(ds.download("sph"), flat.sph)       # spheres survive a rebuild
        osc = O.OracleScene.from_flat(flat)
        lds = ds.kernel_info()["lds_scene"]
        assert lds == fresh.kernel_info()["lds_scene"]
        variants = (LDS_VARIANTS if lds else ()) + GLOBAL_VARIANTS
        for key, (o, d) in list(G.ray_sets(cornell, name.replace("-scattered", "")).items())[:2]:
            check_queries(ds, fresh, osc, f"{name} {key}", o, d, variants, cornell,
                          width=ds.kernel_info()["bvh_arity"] if lds else None, frames=key == "interior" or not lds)
    finally:
        ds.close()
        fresh.close()


# ------------------------------------------------------------------ the point of the feature
def visits_per_query(ds, o, d):
    from pyrenderer_amd import _native as N
    ds.trace_rays(o, d, DEPTH, seed=SEED, flags=N.PRT_FLAG_STATS | variant_flags(3))
    w = ds.diag_words()
    return float(w[N.PRT_DIAG_NODES]) / float(max(int(w[N.PRT_DIAG_EXT]) + int(w[N.PRT_DIAG_SHADOW]), 1)), w


def test_rebuild_tightens_a_scattered_soup(cornell):
    """Recorded on an MI355X: tree cost 9.09 times creation's after the refit and 1.55 times after the rebuild,
    120.5 node visits per query against 25.0 (4.8 times).  The assertion is the ordering only."""
    base = G.scene(cornell, "soup-3000")
    flat = scattered(base)
    o, d = interior(cornell)
    ds = create(base)
    try:
        cost0 = ds.tree_cost()
        ds.update(flat)
        refit_cost = ds.tree_cost()
        refit_visits, w_refit = visits_per_query(ds, o, d)
        ds.rebuild(flat)
        built_cost = ds.tree_cost()
        built_visits, w_built = visits_per_query(ds, o, d)
        print(f"scattered soup-3000: tree cost refit {refit_cost / cost0:.2f} x creation's, rebuilt "
              f"{built_cost / cost0:.2f} x; node visits per query refit {refit_visits:.1f}, rebuilt {built_visits:.1f} "
              f"(ratio {refit_visits / built_visits:.2f})")
        assert int(w_refit[1]) > 0 and int(w_built[0]) > 0
        assert built_visits < refit_visits
        assert built_cost < refit_cost
    finally:
        ds.close()


# ------------------------------------------------------------------ sequences
def test_rebuild_update_update_rebuild(cornell):
    from pyrenderer_amd.flatten import flatten_scene
    moves = cornell_moves(cornell)
    o, d = interior(cornell)
    ds = create(cornell[2])
    try:
        for step, (label, scene) in zip(("rebuild", "update", "update", "rebuild"), moves):
            flat = flatten_scene(scene)
            getattr(ds, step)(flat)
            assert ds.last_update == {"update": "refit", "rebuild": "rebuild"}[step]
            if step == "update":       # a refit of the rebuilt tree: the restated tree's topology with new boxes
                first = L.rebuild(flatten_scene(moves[0][1]).tri_v, 4)
                want = R.refit(first["order"], first["nodes4"], first["nodes8"], flat.tri_v)
                for k in BVH_ORDER:
                    assert not differ(ds.download(k), want[k]), (label, k)
            else:
                check_words(ds, flat, label)
            fresh = create(flat)
            try:
                osc = REFS.get(("osc", label), lambda: O.OracleScene.from_flat(flat))
                v = ds.kernel_info()["variant"]
                assert v == fresh.kernel_info()["variant"]
                check_queries(ds, fresh, osc, label, o, d, (v, 3), cornell, width=ds.kernel_info()["bvh_arity"])
            finally:
                fresh.close()
    finally:
        ds.close()


def test_rebuild_ratio_picks_refit_or_rebuild(cornell):
    """A ratio of 3 lies between the two tree-cost ratios DESIGN.md §13 measured: 1.02 for the spun box, 8.7 for
    the scattered soup."""
    from pyrenderer_amd.flatten import flatten_scene
    ds = create(cornell[2])
    try:
        ds.update(flatten_scene(cornell_moves(cornell)[0][1]), rebuild_ratio=3)
        assert ds.last_update == "refit"
        with pytest.raises(ValueError):
            ds.update(cornell[2], rebuild_ratio=0)
    finally:
        ds.close()
    base = G.scene(cornell, "soup-3000")
    ds = create(base)
    try:
        ds.update(scattered(base), rebuild_ratio=3)
        assert ds.last_update == "rebuild" and ds.rebuild_info()["slots"] == base.n_tri
        ds.update(scattered(base), rebuild_ratio=3)          # the baseline is now the rebuilt tree's
        assert ds.last_update == "refit"
        ds.update(base)
        assert ds.last_update == "refit"
    finally:
        ds.close()


def test_sequence_with_a_rebuild_ratio_equals_a_world_per_frame(cornell):
    """A ratio below 1 rebuilds at every frame, a large one never: both sequences equal the one that builds a
    world per frame, and the accumulator's one device scene says what it did."""
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    from pyrenderer_amd.scenes import spun
    scene, cam, _ = cornell
    scenes = spun(scene, 5, 6.0, 3)
    kw = dict(spp=1, depth=DEPTH, seed=SEED, resolution=(W, H), scenes=scenes)
    per_frame = render_sequence(scene, [cam] * 3, refit=False, **kw)
    for ratio, did in ((0.5, "rebuild"), (100.0, "refit")):
        assert not differ(render_sequence(scene, [cam] * 3, refit=True, rebuild_ratio=ratio, **kw), per_frame), ratio
        acc = TemporalAccumulator(scene, depth=DEPTH, spp=1, seed=SEED, resolution=(W, H), refit=True, rebuild_ratio=ratio)
        for s in scenes:
            acc.add(cam, s)
        assert acc.world.device_scene(0).last_update == did
        for ds in acc.world.device_scenes.values():
            ds.close()


# ------------------------------------------------------------------ edge cases on the device
def tiny_flat(cornell, tri_v):
    """A scene of the given triangles, all of Cornell's first material but triangle 0, which is the light."""
    from pyrenderer_amd.flatten import FlatScene
    c = cornell[2]
    n = tri_v.shape[0]
    v = tri_v.reshape(n, 3, 3).astype(np.float32)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = (nrm / np.where(length > 0, length, 1)).astype(np.float32)
    light_mat = int(c.tri_mat[c.light_tri[0]])
    other = int(np.flatnonzero(np.arange(c.mat.shape[0]) != light_mat)[0])
    tri_mat = np.full(n, other, np.int32)
    tri_mat[0] = light_mat
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    return FlatScene(np.ascontiguousarray(v.reshape(n, 9)), nrm, tri_mat, np.zeros(n, np.int32),
                     lo[None].astype(np.float32), hi[None].astype(np.float32), c.mat, np.zeros(1, np.int32),
                     np.array([0, 1], np.int32), c.direct_rgb, np.zeros((0, 4), np.float32), np.zeros(0, np.int32),
                     np.zeros(0, np.int32))


def rays_at(tri_v, n=256, seed=3):
    """Rays from above the triangles' bounds aimed at points inside them."""
    rng = np.random.default_rng(seed)
    p = tri_v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    ext = max(float((hi - lo).max()), 1.0)
    target = lo + rng.random((n, 3)) * (hi - lo)
    origin = target + np.array([0.1, 0.2, 1.0]) * 2 * ext + rng.normal(size=(n, 3)) * 0.05 * ext
    d = target - origin
    return origin.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("name", ["one", "three", "duplicates", "plane"])
def test_edge_cases_on_the_device(cornell, name):
    tri_v = L.edge_case(L.one_triangle(), name)      # duplicates: of a triangle with an area
    flat = tiny_flat(cornell, tri_v)
    ds = create(flat)
    try:
        lds = ds.kernel_info()["lds_scene"]        # the larger shapes are past what the LDS kernels hold
        ds.rebuild(flat)
        assert ds.kernel_info()["lds_scene"] == lds
        want = check_words(ds, flat, f"edge {name}", lds=lds)
        if name in ("one", "three"):
            assert want["nodes4"].shape[0] == 1 and ds.rebuild_info()["need4"] == 4
        osc = O.OracleScene.from_flat(flat)
        o, d = rays_at(tri_v)
        wid, wt = osc.closest(o, d, T_MIN, T_MAX)[:2]
        assert int((np.asarray(wid) != 0).sum()) > 0
        for quantized in (False, True):
            n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized, False)
            assert n == 0, (name, quantized, n, bad)
        if name == "duplicates":
            gid, _ = ds.closest_hits(o, d, T_MIN, T_MAX)
            assert set(np.unique(gid).tolist()) <= {-1, 0}        # the lowest id wins every tie
        ds.check_faults()
    finally:
        ds.close()


def test_sphere_only_scene(cornell):
    """No triangle at all is not a scene the library accepts (a light is a triangle); the nearest thing is one
    light triangle beside spheres, and the empty range is restated on the CPU (tests/test_lbvh_ref.py)."""
    from kernel_parity import specular_scene
    flat = specular_scene()[2]
    assert flat.sph.shape[0] >= 1
    o, d = interior(cornell)
    ds = create(flat)
    fresh = create(flat)
    try:
        ds.rebuild(flat)
        assert not differ(ds.download("sph"), flat.sph)
        osc = O.OracleScene.from_flat(flat)
        want = REFS.closest("spheres", osc, o, d)
        n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, False, False, want=want)
        assert n == 0, bad
        v = ds.kernel_info()["variant"]
        assert not differ(frame_of(ds, cornell, v), frame_of(fresh, cornell, v))
        ds.check_faults()
    finally:
        ds.close()
        fresh.close()


# ------------------------------------------------------------------ survival and refusal
def test_render_contexts_survive_a_rebuild(cornell):
    import torch
    from pyrenderer_amd.flatten import flatten_scene
    flat = flatten_scene(cornell_moves(cornell)[0][1])
    cam = packed_camera(cornell)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    outs = [torch.empty(len(IDS) * TILE * TILE * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    ds = create(cornell[2])
    fresh0, fresh = create(cornell[2]), create(flat)
    try:
        ds.render_tiles_device(cam, W, H, TILE, TILE, IDS, SPP, DEPTH, outs[0].data_ptr(), stream.cuda_stream, seed=SEED)
        ds.rebuild(flat)      # synchronises the device first: the render above has finished
        ds.render_tiles_device(cam, W, H, TILE, TILE, IDS, SPP, DEPTH, outs[1].data_ptr(), stream.cuda_stream, seed=SEED)
        stream.synchronize()
        ds.check_faults()
        first, second = (t.cpu().numpy().reshape(-1, 3) for t in outs)
        assert not differ(first, frame_of(fresh0, cornell))
        assert not differ(second, frame_of(fresh, cornell))
        assert differ(first, second)
    finally:
        ds.close()
        fresh0.close()
        fresh.close()


def test_refused_rebuild_leaves_the_scene_as_it_was(cornell):
    from pyrenderer_amd import _native as N
    flat0 = cornell[2]
    ds = create(flat0)
    try:
        ds.rebuild(flat0)
        names = BVH_ORDER + ORIGINAL_ORDER
        before = {k: ds.download(k) for k in names}
        frame = frame_of(ds, cornell)
        nan = flat0.tri_v.copy()
        nan[flat0.n_tri // 2, 4] = np.nan
        with pytest.raises(N.PrtError) as e:
            ds.rebuild(with_geometry(flat0, tri_v=nan))
        assert e.value.code == N.PRT_ERR_ARG and ds.flat is flat0
        L_ = N.lib()
        assert L_.prt_scene_rebuild(ds.h, None, N.ptr(flat0.tri_n), None) == N.PRT_ERR_ARG
        assert L_.prt_scene_rebuild(ds.h, N.ptr(flat0.tri_v), None, None) == N.PRT_ERR_ARG
        with pytest.raises(ValueError):
            ds.rebuild(G.scene(cornell, "soup-zoo"))             # other counts
        for k in names:
            assert not differ(ds.download(k), before[k]), k
        assert not differ(frame_of(ds, cornell), frame)
    finally:
        ds.close()

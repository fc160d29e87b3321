"""prt_scene_update on the GPU: a resident scene whose primitives moved is refit on the
device and must then hold, word for word, what tests/refit_ref.py computes from the creation-time tree and the
new vertices, and render, bit for bit, what a scene freshly created from the same arrays renders and what the
oracle's brute-force backend gives — through every trace-kernel variant, both tree widths of the LDS kernels,
the f32 and the quantised hit queries.  Results do not depend on the tree (ties go to the lowest id), so the
bound on every comparison is equality."""
import numpy as np
import pytest

import global_cases as G
import refit_ref as R
from kernel_parity import (T_MAX, T_MIN, OracleRefs, all_tiles, check_trace, hits_wrong, is_mis, packed_camera,
                           random_bounds, specular_scene, variant_flags)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NO_SPLITS = {"PRT_SBVH": 0, "PRT_ESC_BETA": 0}
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


def built_tree(flat, setting):
    """The creation-time tree of `flat` under `setting`, as the restatement takes it."""
    from pyrenderer_amd._native import Bvh
    with G.knobs(setting):
        b = Bvh(flat.tri_v)
        order = b.export()[2]
        return dict(order=order, nodes4=b.collapse(4)[0], nodes8=b.collapse(8)[0], pad=np.float32(b.pad))


def create(flat, setting):
    from pyrenderer_amd.device_scene import DeviceScene
    with G.knobs(setting):
        return DeviceScene(flat, 0)


def with_geometry(flat, tri_v=None, tri_n=None, sph=None):
    from pyrenderer_amd.flatten import FlatScene
    return FlatScene(flat.tri_v if tri_v is None else tri_v, flat.tri_n if tri_n is None else tri_n, flat.tri_mat,
                     flat.tri_prim, flat.prim_lo, flat.prim_hi, flat.mat, flat.light_tri, flat.light_off,
                     flat.direct_rgb, flat.sph if sph is None else sph, flat.sph_mat, flat.sph_prim)


def interior(cornell):
    return G.ray_sets(cornell, "soup-3000")["interior"]


def frame_of(ds, cornell, v=0):
    img, _ = ds.render_tiles(packed_camera(cornell), W, H, TILE, TILE, IDS, SPP, DEPTH, SEED, variant_flags(v) if v else 0)
    ds.check_faults()
    return img


def oracle_frame(key, osc, cornell, mis=False):
    return REFS.render_tiles(key, osc, packed_camera(cornell), W, H, TILE, IDS, SPP, DEPTH, SEED, mis=mis)[0]


def check_queries(ds, fresh, osc, key, o, d, variants, cornell, width=None):
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
        check_trace(ds, ref, o, d, DEPTH, SEED, v, label=f"{key} v{v}", width=width if v in LDS_VARIANTS else None)
        img = frame_of(ds, cornell, v)
        assert not differ(img, oracle_frame(key, osc, cornell, is_mis(v))), (key, v, "frame against the oracle")
        assert not differ(img, frame_of(fresh, cornell, v)), (key, v, "frame against the fresh scene")
    ds.check_faults()


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize("name", ["cornell", "soup-3000"])
def test_update_with_the_same_geometry_changes_no_word(cornell, name):
    flat = cornell[2] if name == "cornell" else G.scene(cornell, name)
    ds = create(flat, NO_SPLITS)
    try:
        names = BVH_ORDER if name == "cornell" else BVH_ORDER[:3]
        before = {k: ds.download(k) for k in names + ORIGINAL_ORDER}
        assert before["tris"].shape[0] == flat.n_tri and before["nodes4"].shape[0] >= 1
        if name == "cornell":
            assert before["nodes8"].shape[0] >= 1
        # the created quantised nodes pin the NumPy quantiser
        t = built_tree(flat, NO_SPLITS)
        assert not differ(before["nodes4"], t["nodes4"])
        assert not differ(R.quantize4(before["nodes4"], t["pad"]), before["nodes4q"])
        created_bytes = ds.device_bytes
        ds.update(flat)
        # the first update allocates the order, level lists, slot bounds and vertices; a second one nothing
        grown = ds.device_bytes
        assert grown >= created_bytes + 4 * 16 * flat.n_tri, (created_bytes, grown)
        assert ds.update(flat).device_bytes == grown
        for k, b in before.items():
            assert not differ(ds.download(k), b), (name, k, differ(ds.download(k), b))
        ms = ds.download("update_ms")[0]
        assert ms.shape == (5,) and (ms >= 0).all() and np.isfinite(ms).all()
        ds.check_faults()
    finally:
        ds.close()


# ------------------------------------------------------------------ the moved Cornell box
def cornell_moves(cornell):
    """[(label, scene)]: the short box (primitive 5) spun 6 degrees three times, cumulatively, then the tall box
    (6) carried outside the room's bounding box, so that the pad, the root box and the quantisation origins move."""
    from pyrenderer_amd.scenes import moved, spun
    spins = spun(cornell[0], 5, 6.0, 4)[1:]
    g = np.eye(4)
    g[0, 3] = 3.0
    return [(f"spin-{k + 1}", s) for k, s in enumerate(spins)] + [("tall-out", moved(spins[-1], {6: g}))]


@pytest.mark.parametrize("width", [4, 8])
def test_moved_cornell(cornell, width):
    from pyrenderer_amd.flatten import flatten_scene
    flat0 = cornell[2]
    setting = {"PRT_LDS_WIDTH": width}
    tree = built_tree(flat0, setting)
    o, d = interior(cornell)
    ds = create(flat0, setting)
    try:
        assert ds.kernel_info()["lds_scene"] and ds.download("nodes8").shape[0] >= 1
        cost0 = ds.tree_cost()
        pads = {float(tree["pad"])}
        for label, scene in cornell_moves(cornell):
            flat = flatten_scene(scene)
            assert flat.tri_v.tobytes() != ds.flat.tri_v.tobytes()
            assert ds.update(flat) is ds and ds.flat is flat
            want = R.refit(tree["order"], tree["nodes4"], tree["nodes8"], flat.tri_v)
            pads.add(float(want["pad"]))
            for k in BVH_ORDER:
                assert not differ(ds.download(k), want[k]), (label, k, differ(ds.download(k), want[k]))
            fresh = create(flat, setting)
            try:
                for k in ORIGINAL_ORDER:
                    assert not differ(ds.download(k), fresh.download(k)), (label, k)
                for k in ("variant", "lds_scene", "shade_fast", "plain"):     # the stack is the tree's own
                    assert ds.kernel_info()[k] == fresh.kernel_info()[k], (label, k)
                osc = REFS.get(("osc", label), lambda: O.OracleScene.from_flat(flat))
                check_queries(ds, fresh, osc, label, o, d, LDS_VARIANTS + GLOBAL_VARIANTS, cornell, width=width)
            finally:
                fresh.close()
            print(f"{label} width {width}: tree cost {ds.tree_cost() / cost0:.3f} of creation's")
        assert len(pads) >= 2      # the last move changed the pad
        root_hi_x = ds.download("nodes4")[0, 4:8]
        assert root_hi_x[np.isfinite(root_hi_x)].max() > 2.0      # ... and the root's box
    finally:
        ds.close()


def test_moved_light(cornell):
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.scenes import moved
    g = np.eye(4)
    g[1, 3] = -0.1
    flat = flatten_scene(moved(cornell[0], {7: g}))
    assert flat.tri_v[cornell[2].light_tri].tobytes() != cornell[2].tri_v[cornell[2].light_tri].tobytes()
    ds = create(cornell[2], {})
    try:
        before = frame_of(ds, cornell)
        ds.update(flat)
        img = frame_of(ds, cornell)
        assert differ(img, before)
        osc = O.OracleScene.from_flat(flat)
        assert not differ(img, oracle_frame("light", osc, cornell))
        for v in GLOBAL_VARIANTS:
            assert not differ(frame_of(ds, cornell, v), oracle_frame("light", osc, cornell, is_mis(v))), v
    finally:
        ds.close()


def test_moved_sphere(cornell):
    flat0 = specular_scene()[2]
    assert flat0.sph.shape[0] >= 1
    sph = flat0.sph.copy()
    sph[0, :3] += np.array([0.2, 0.15, -0.1], np.float32)
    flat = with_geometry(flat0, sph=sph)
    o, d = interior(cornell)
    ds = create(flat0, {})
    try:
        ds.update(flat)
        assert not differ(ds.download("sph"), sph)
        osc = O.OracleScene.from_flat(flat)
        info = ds.kernel_info()
        for v in (info["variant"], 3):
            ref = REFS.trace("sphere", osc, o, d, DEPTH, SEED, False)
            check_trace(ds, ref, o, d, DEPTH, SEED, v, label=f"sphere v{v}", finite=bool(np.isfinite(ref).all()))
        want = REFS.closest("sphere", osc, o, d)
        n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, False, False, want=want)
        assert n == 0, bad
    finally:
        ds.close()


# ------------------------------------------------------------------ references split at creation
def test_splits_on_stays_conservative_and_exact(cornell):
    flat0 = G.scene(cornell, "soup-3000")
    tree = built_tree(flat0, {})
    assert tree["order"].size > flat0.n_tri
    flat = with_geometry(flat0, tri_v=R.displaced(flat0.tri_v))
    ds = create(flat0, {})
    try:
        ds.update(flat)
        nodes4, tris = ds.download("nodes4"), ds.download("tris")
        want = R.refit(tree["order"], tree["nodes4"], None, flat.tri_v)
        assert not differ(nodes4, want["nodes4"]) and not differ(tris, want["tris"])
        assert not differ(ds.download("nodes4q"), want["nodes4q"])
        assert R.containment(nodes4, 4, tree["order"], flat.tri_v, want["pad"]) == (0, 0)
        osc = O.OracleScene.from_flat(flat)
        for key, (o, d) in G.ray_sets(cornell, "soup-3000").items():
            label = f"displaced {key}"
            want_hits = REFS.closest(label, osc, o, d)
            for quantized in (False, True):
                n, bad, _ = hits_wrong(ds, osc, o, d, T_MIN, T_MAX, quantized, False, want=want_hits)
                assert n == 0, (label, quantized, n, bad)
            for v in GLOBAL_VARIANTS:
                ref = REFS.trace(label, osc, o, d, DEPTH, SEED, is_mis(v))
                check_trace(ds, ref, o, d, DEPTH, SEED, v, label=f"{label} v{v}", lds_scene=False,
                            finite=True)
        ds.check_faults()
    finally:
        ds.close()


# ------------------------------------------------------------------ shade_fast, contexts, errors
def test_shade_fast_follows_the_normals(cornell):
    flat0 = cornell[2]
    long = with_geometry(flat0, tri_n=(flat0.tri_n * np.float32(3.0)).astype(np.float32))
    o, d = interior(cornell)
    ds = create(flat0, {})
    try:
        assert ds.kernel_info()["shade_fast"]
        ds.update(long)
        info = ds.kernel_info()
        assert not info["shade_fast"]
        osc = O.OracleScene.from_flat(long)
        ref = REFS.trace("normals-3", osc, o, d, DEPTH, SEED, False)
        check_trace(ds, ref, o, d, DEPTH, SEED, info["variant"], label="normals x 3", expect={"shade_fast": False})
        ds.update(flat0)
        assert ds.kernel_info()["shade_fast"]
        ref = REFS.trace("normals-1", REFS.get(("osc", "cornell"), lambda: O.OracleScene.from_flat(flat0)), o, d, DEPTH,
                         SEED, False)
        check_trace(ds, ref, o, d, DEPTH, SEED, info["variant"], label="normals back", expect={"shade_fast": True})
    finally:
        ds.close()


def test_render_contexts_survive(cornell):
    import torch
    from pyrenderer_amd.flatten import flatten_scene
    flat = flatten_scene(cornell_moves(cornell)[0][1])
    cam = packed_camera(cornell)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    outs = [torch.empty(len(IDS) * TILE * TILE * 3, dtype=torch.float32, device=dev) for _ in range(2)]
    ds = create(cornell[2], {})
    fresh = create(flat, {})
    try:
        ds.render_tiles_device(cam, W, H, TILE, TILE, IDS, SPP, DEPTH, outs[0].data_ptr(), stream.cuda_stream, seed=SEED)
        ds.update(flat)      # synchronises the device first: the render above has finished
        ds.render_tiles_device(cam, W, H, TILE, TILE, IDS, SPP, DEPTH, outs[1].data_ptr(), stream.cuda_stream, seed=SEED)
        stream.synchronize()
        ds.check_faults()
        first, second = (t.cpu().numpy().reshape(-1, 3) for t in outs)
        assert differ(first, second)
        assert not differ(second, frame_of(fresh, cornell))
    finally:
        ds.close()
        fresh.close()


def test_errors_leave_the_scene_as_it_was(cornell):
    from pyrenderer_amd import _native as N
    flat0 = specular_scene()[2]
    ds = create(flat0, {})
    try:
        before = frame_of(ds, cornell)
        nan = flat0.tri_v.copy()
        nan[flat0.n_tri // 2, 4] = np.nan
        zero = flat0.sph.copy()
        zero[0, 3] = 0.0
        for bad in (with_geometry(flat0, tri_v=nan), with_geometry(flat0, sph=zero)):
            with pytest.raises(N.PrtError) as e:
                ds.update(bad)
            assert e.value.code == N.PRT_ERR_ARG
            assert ds.flat is flat0
            assert not differ(frame_of(ds, cornell), before)
        with pytest.raises(ValueError):
            ds.update(cornell[2])                       # other counts
        other = with_geometry(flat0)
        other.tri_mat = flat0.tri_mat[::-1].copy()
        with pytest.raises(ValueError):
            ds.update(other)
        lights = with_geometry(flat0)
        lights.light_tri = (flat0.light_tri[::-1]).copy()
        with pytest.raises(ValueError):
            ds.update(lights)
        assert not differ(frame_of(ds, cornell), before)
        with pytest.raises(N.PrtError):
            out = np.zeros(3, np.float32)
            N.check(N.lib().prt_scene_download(ds.h, N.PRT_BUF_NODES4, N.ptr(out), out.nbytes))
    finally:
        ds.close()


# ------------------------------------------------------------------ the sequence API
def test_sequence_refit_equals_rebuild(cornell):
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    from pyrenderer_amd.scenes import spun
    scene, cam, _ = cornell
    scenes = spun(scene, 5, 6.0, 4)
    kw = dict(spp=1, depth=DEPTH, seed=SEED, resolution=(W, H), scenes=scenes)
    rebuilt = render_sequence(scene, [cam] * 4, refit=False, **kw)
    refit = render_sequence(scene, [cam] * 4, refit=True, **kw)
    assert rebuilt.shape == (4, W, H, 3) and not differ(refit, rebuilt)
    assert differ(rebuilt[0], rebuilt[3])
    for flag, same in ((True, True), (False, False)):
        acc = TemporalAccumulator(scene, depth=DEPTH, spp=1, seed=SEED, resolution=(W, H), refit=flag)
        seen = []
        for s in scenes:
            acc.add(cam, s)
            seen.append(acc.world.device_scene(0))
        assert all(ds is seen[0] for ds in seen) == same, flag
        assert seen[-1].flat.tri_v.tobytes() == acc.world.flat.tri_v.tobytes()
        for ds in acc.world.device_scenes.values():
            ds.close()


def test_static_frame_then_moving_refit_equals_rebuild(cornell):
    """add(cam) then add(cam, moved): the static frame kept no id plane, so the previous frame's plane is composed
    when the moving frame arrives.  It has to show the previous pose although the refit moves the one device
    scene in place: state, colour and this frame's ids equal the rebuild's, bit for bit."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import TemporalAccumulator
    from pyrenderer_amd.scenes import spun
    scene, cam, _ = cornell
    moved_scene = spun(scene, 5, 6.0, 4)[3]
    got = {}
    for flag in (False, True):
        acc = TemporalAccumulator(scene, depth=DEPTH, spp=1, seed=SEED, resolution=(W, H), refit=flag)
        acc.add(cam)
        first = acc.world.device_scene(0)
        before = D.object_ids(first, acc.frame.cam, W, H).copy()
        acc.add(cam, moved_scene)
        assert (acc.world.device_scene(0) is first) == flag
        after = acc.object_ids()
        assert int((before != after).sum()) > 0      # the two poses' planes differ: the wrong one would show
        got[flag] = (acc.state().copy(), acc.accumulated().copy(), after.copy(), acc.history().copy())
        for ds in acc.world.device_scenes.values():
            ds.close()
    for k, (a, b) in enumerate(zip(got[True], got[False])):
        assert not differ(a, b), (k, differ(a, b))
    assert int((got[True][3] > 1).sum()) > 0 and int((got[True][3] == 1).sum()) > 0   # history kept and restarted

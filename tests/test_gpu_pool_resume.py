"""Suspended extension-traversal tails in the pooled trace kernel (TraceParams::pool_resume_min, env
PRT_POOL_RESUME_MIN read at scene creation): a wave leaves its extension traversal once
at most the threshold lanes are still traversing, the unfinished lanes resume their query in the
next iteration.  Which lane finishes when must not change a bit: every render here equals the
threshold-0 render and the C oracle bit for bit, trips no watchdog (prt_check_faults) and produces no
non-finite sample; the STATS build's suspension counter (diag word 176) shows that the path ran."""
import numpy as np
import pytest

from kernel_parity import all_tiles, open_scenes, packed_camera, render_twice, scene_json, specular_scene
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes_by_threshold():
    """make(name, flat, threshold) -> DeviceScene created with PRT_POOL_RESUME_MIN = threshold (cached)."""
    with open_scenes() as make:
        yield lambda name, flat, thr: make(name, flat, PRT_POOL_RESUME_MIN=thr)


def _render(ds, cam, W, H, tile, ids, spp, depth, seed, variant=0):
    """(image of the production and the STATS build, (ext, shadow) query counts, suspensions, resumes)."""
    from pyrenderer_amd import _native as N
    r = render_twice(ds, cam, W, H, tile, ids, spp, depth, seed, variant << 8)
    return r["img"], r["queries"], int(r["words"][N.PRT_DIAG_SUSPENDED]), int(r["words"][N.PRT_DIAG_RESUMED])


def _check(make, name, flat, cam, W, H, tile, spp, depth, seed, thresholds, variant=0, expect_suspensions=True):
    ids = all_tiles(W, H, tile)
    ref, cnt = O.OracleScene.from_flat(flat).render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed=seed,
                                                          counters=True)
    assert make(name, flat, 0).kernel_info(len(ids) * tile * tile * spp, variant << 8)["variant"] == (variant or 7)
    base, q0, s0, r0 = _render(make(name, flat, 0), cam, W, H, tile, ids, spp, depth, seed, variant)
    assert (s0, r0) == (0, 0)
    assert np.array_equal(base, ref)
    assert q0 == (int(cnt[2]), int(cnt[3]))
    for thr in thresholds:
        img, q, ns, nr = _render(make(name, flat, thr), cam, W, H, tile, ids, spp, depth, seed, variant)
        print(f"{name} {W}x{H}x{spp} depth {depth} threshold {thr}: {ns} suspensions, {nr} resumes, "
              f"{q[0]} ext / {q[1]} shadow queries, {int((img != ref).any(axis=-1).sum())} pixels differ")
        assert np.array_equal(img, base) and np.array_equal(img, ref), thr
        assert q == (int(cnt[2]), int(cnt[3])), thr     # a resumed query is counted once
        assert ns == nr, thr                            # every suspended query was resumed
        if expect_suspensions:
            assert ns > 0, thr


def test_threshold_sweep(scenes_by_threshold, cornell):
    """4.2 M items, about nine per resident lane: suspension in steady state.  64 suspends whenever any
    lane is unfinished."""
    cam = packed_camera(cornell)
    _check(scenes_by_threshold, "cornell", cornell[2], cam, 256, 256, 64, 64, 8, 2, (1, 8, 16, 64))


def test_specular_scene(scenes_by_threshold):
    """The full build: the sphere is tested once, when the query completes; metal and dielectric paths."""
    _, cam, flat = specular_scene(0.35)
    assert flat.sph.shape[0] == 1
    _check(scenes_by_threshold, "specular", flat, cam.convert_to_taichi_camera().packed(), 128, 128, 64, 32, 8, 4,
           (16, 64))


@pytest.mark.parametrize("depth", [1, 2])
def test_short_paths(scenes_by_threshold, cornell, depth):
    """Paths ended by their pending shadow ray (no extension query in their last iteration)."""
    cam = packed_camera(cornell)
    _check(scenes_by_threshold, "cornell", cornell[2], cam, 256, 256, 64, 16, depth, 5, (64,))


def test_ragged_frame(scenes_by_threshold, cornell):
    """A width and height that are no multiple of the tile: lanes that drew a slot outside the frame."""
    cam = packed_camera(cornell)
    _check(scenes_by_threshold, "cornell", cornell[2], cam, 200, 136, 64, 32, 8, 6, (16, 64))


def test_multi_frame_launch(scenes_by_threshold, cornell, oracle_scene):
    """Three progressive frames through one persistent launch."""
    import torch
    cam = packed_camera(cornell)
    W = H = 128
    tile, spp, depth, n, seed = 64, 32, 8, 3, 7
    ids = all_tiles(W, H, tile)
    n_slots = len(ids) * tile * tile
    frames = {}
    for thr in (0, 16, 64):
        ds = scenes_by_threshold("cornell", cornell[2], thr)
        out = torch.full((n, n_slots * 3), float("nan"), dtype=torch.float32, device="cuda:0")
        ds.render_frames_device(cam, W, H, tile, tile, ids, spp, depth, n, out.data_ptr(), None, seed=seed,
                                frame_stride=spp)
        ds.check_faults()
        frames[thr] = out.cpu().numpy().reshape(n, n_slots, 3)
    assert np.array_equal(frames[0][0], oracle_scene.render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed=seed))
    for f in range(n):
        ref = np.zeros((n_slots, 3), np.float32)
        scenes_by_threshold("cornell", cornell[2], 0).render_tiles_accumulate(cam, W, H, tile, tile, ids, f * spp, spp,
                                                                              depth, ref, seed=seed)
        for thr in (0, 16, 64):
            assert np.array_equal(frames[thr][f], ref), (thr, f)


def test_multi_light(scenes_by_threshold, tmp_path):
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    scene, cam = read_file(scene_json(tmp_path))
    flat = flatten_scene(scene)
    assert flat.n_light == 3
    # this scene's LDS copy does not fit seven blocks per CU beside the pool (its default is the
    # phase-aligned kernel): the pooled kernel forced, at the occupancy it gets
    _check(scenes_by_threshold, "lights", flat, cam.convert_to_taichi_camera().packed(), 128, 128, 64, 32, 8, 8, (16,),
           variant=N.VAR_LDS_POOL)


def test_small_launch(scenes_by_threshold, cornell):
    """8192 items, fewer than the resident lanes: the queue is exhausted at once, and the threshold has
    no effect on the image."""
    cam = packed_camera(cornell)
    _check(scenes_by_threshold, "cornell", cornell[2], cam, 64, 64, 64, 2, 8, 9, (16, 64), variant=7,
           expect_suspensions=False)


def test_six_wave_build(scenes_by_threshold, cornell):
    from pyrenderer_amd import _native as N
    cam = packed_camera(cornell)
    _check(scenes_by_threshold, "cornell", cornell[2], cam, 256, 256, 64, 16, 8, 11, (16,), variant=N.VAR_LDS_POOL6)

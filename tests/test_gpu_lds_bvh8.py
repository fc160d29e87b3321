"""The eight-wide tree of LDS-resident scenes in the trace kernels (visit_node8; env PRT_LDS_WIDTH read at
scene creation forces the width).  The closest (t, id) and every any-hit answer do not
depend on the visiting order, so a width-8 render equals the width-4 render of the same build and the C
oracle bit for bit, asks the same number of extension and shadow queries, trips no watchdog and produces
no non-finite sample."""
import numpy as np
import pytest

import bvh8_scenes as S8
from kernel_parity import all_tiles, packed_camera, render_twice, specular_scene
from kernel_parity import scenes_by_width as scenes  # noqa: F401  (the module-scoped fixture)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEFAULT_WIDTH = 8   # of a scene that can take either (prt_plan.cpp lds_width)


def _check(make, name, flat, cam, W, H, spp, depth, seed, variant=0, ids=None, tile=64):
    ids = all_tiles(W, H, tile) if ids is None else np.asarray(ids, np.int32)
    ref, cnt = O.OracleScene.from_flat(flat).render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed=seed,
                                                          counters=True)
    r4, r8 = (render_twice(make(name, flat, w), cam, W, H, tile, ids, spp, depth, seed, variant << 8, width=w)
              for w in (4, 8))
    (img4, q4), (img8, q8) = (r4["img"], r4["queries"]), (r8["img"], r8["queries"])
    print(f"{name} {W}x{H}x{spp} depth {depth} variant {variant}: {q8[0]} ext / {q8[1]} shadow queries, "
          f"{int((img8 != img4).any(axis=-1).sum())} pixels differ from width 4, "
          f"{int((img8 != ref).any(axis=-1).sum())} from the oracle")
    assert np.array_equal(img8, img4) and np.array_equal(img8, ref)
    assert q8 == q4 == (int(cnt[2]), int(cnt[3]))


def test_cornell(scenes, cornell):
    _check(scenes, "cornell", cornell[2], packed_camera(cornell), 64, 64, 4, 8, 3)


def test_specular_scene(scenes):
    """The pooled kernel's full build: a sphere, metal and dielectric paths."""
    _, cam, flat = specular_scene(0.35)
    assert flat.sph.shape[0] == 1
    _check(scenes, "specular", flat, cam.convert_to_taichi_camera().packed(), 32, 32, 4, 8, 4)


@pytest.mark.parametrize("name", ["five", "nine-leaves"])
def test_small_trees(scenes, cornell, name):
    """A root whose children are all leaves (five of its eight slots empty), and a root with one inner child."""
    flat = S8.five_triangles(cornell[2]) if name == "five" else S8.nine_leaves(cornell[2])
    _check(scenes, name, flat, packed_camera(cornell), 32, 32, 2, 8, 5)


def test_ragged_tile_set(scenes, cornell):
    """A frame that is no multiple of the tile, and three of its four tiles."""
    _check(scenes, "cornell", cornell[2], packed_camera(cornell), 100, 72, 4, 8, 6, ids=[0, 1, 3])


def test_phase_aligned_kernel(scenes, cornell):
    """trace_kernel's LDS instantiation over the eight-wide tree (variant forced)."""
    from pyrenderer_amd import _native as N
    _check(scenes, "cornell", cornell[2], packed_camera(cornell), 64, 64, 4, 8, 3, variant=N.VAR_LDS)


def test_multi_frame_launch(scenes, cornell, oracle_scene):
    """Three progressive frames through one persistent launch."""
    import torch
    cam = packed_camera(cornell)
    W = H = 64
    tile, spp, depth, n, seed = 64, 4, 8, 3, 7
    ids = all_tiles(W, H, tile)
    n_slots = len(ids) * tile * tile
    frames = {}
    for width in (4, 8):
        ds = scenes("cornell", cornell[2], width)
        out = torch.full((n, n_slots * 3), float("nan"), dtype=torch.float32, device="cuda:0")
        ds.render_frames_device(cam, W, H, tile, tile, ids, spp, depth, n, out.data_ptr(), None, seed=seed,
                                frame_stride=spp)
        ds.check_faults()
        frames[width] = out.cpu().numpy().reshape(n, n_slots, 3)
    assert np.array_equal(frames[8], frames[4])
    assert np.array_equal(frames[8][0], oracle_scene.render_tiles(cam, W, H, tile, tile, ids, spp, depth, seed=seed))
    assert not np.array_equal(frames[8][1], frames[8][0])


def test_suspended_tails(scenes, cornell):
    """PRT_POOL_RESUME_MIN at width 8: the parked state (node, leaf, stack pointer, best hit) is the same
    words for either tree.  1 M items, two per resident lane, so that the thresholds apply."""
    from pyrenderer_amd import _native as N
    cam = packed_camera(cornell)
    W = H = 256
    ids = all_tiles(W, H, 64)
    got = {thr: render_twice(scenes("cornell", cornell[2], 8, PRT_POOL_RESUME_MIN=thr), cam, W, H, 64, ids, 16, 8, 2, 0,
                             width=8) for thr in (0, 1, 64)}
    base4 = render_twice(scenes("cornell", cornell[2], 4, PRT_POOL_RESUME_MIN=0), cam, W, H, 64, ids, 16, 8, 2, 0,
                         width=4)
    suspended = {thr: int(g["words"][N.PRT_DIAG_SUSPENDED]) for thr, g in got.items()}
    print(suspended)
    assert suspended[0] == 0 and suspended[64] > 0
    for thr in (1, 64):
        assert np.array_equal(got[thr]["img"], got[0]["img"]) and got[thr]["queries"] == got[0]["queries"], thr
    assert np.array_equal(got[0]["img"], base4["img"]) and got[0]["queries"] == base4["queries"]


def test_info_call_reports_the_width(scenes, cornell):
    from pyrenderer_amd import _native as N
    flat = cornell[2]
    assert scenes("cornell", flat, None).kernel_info()["bvh_arity"] == DEFAULT_WIDTH
    ds8 = scenes("cornell", flat, 8)
    k = ds8.kernel_info()
    assert (k["variant"], k["bvh_arity"], k["stack"]) == (N.VAR_LDS_POOL, 8, 15), k
    # the MIS estimator's LDS kernel keeps the BVH4
    assert ds8.kernel_info(64 * 64 * 4, N.PRT_FLAG_MIS_NEE)["bvh_arity"] == 4
    # a scene whose eight-wide tree needs more than the pooled kernel's 32 stack entries keeps the BVH4,
    # whatever the knob says
    deep = S8.chain(flat)
    for width in (None, 8):
        kd = scenes("chain", deep, width, PRT_MAX_LEAF=S8.CHAIN_MAX_LEAF).kernel_info()
        assert kd["lds_scene"] and kd["bvh_arity"] == 4, kd

"""The global-scene trace kernel (variants 3 and 5: quantised BVH4 in HBM, LDS stack with its global spill,
suspended traversal tails) under every schedule threshold in steady state and over every tree shape the
builder's knobs produce, bit for bit against the oracle's brute-force backend.  No tolerance anywhere.

Why the older launches never exercised the thresholds in steady state.  The kernel's loop (prt_trace.h)
passes leaf_break, leaf_exit and resume_min to traverse_ww4 only while no chunk claim of the wave has
failed; once one fails (`exhausted`) all three are 0 for the rest of the launch.  A launch of 4096 caller
rays or of a 64 x 64 x 4 frame is smaller than the lanes one GPU keeps resident (blocks_per_cu * CUs * 256,
393 216 on an MI355X at six blocks per CU): a wave claims once, runs its first queries under the
thresholds, and is exhausted at its first refill, when the first of its paths has ended.  Such a launch
does suspend and resume queries at its head (a mutant that loses `best` over a suspension fails the older
small-launch tests too), but it never refills a lane, so a resumed query never sits beside a fresh path,
shadow and extension queries of different generations never share a wave, and most of every path runs
with thresholds 0 whatever PRT_RESUME_MIN, PRT_LEAF_BREAK and PRT_LEAF_EXIT say; none of those tests sets
them anyway.  Part A renders at least FACTOR = 4 items per resident lane (asserted from the scene's own
occupancy), so that for most of the launch the wave is refilled and the thresholds under test apply.

Why every outer trip of traverse_ww4 makes progress at leaf_break = leaf_exit = 64 (prt_traverse.h, the
do-while).  State at the top of a trip: `cur` (>= 0 an inner node, < 0 a leaf, kSent = the stack ran
empty), `leaf` (< 0 a postponed leaf, >= 0 none).  (a) `cur < 0 && leaf >= 0` cannot stand at the top of
a trip: tstate_init starts at the root (or kSent), the node phase turns that state into a postponed leaf
at once (leaf = cur, cur = pop), and the leaf phase ends each of its trips with leaf = cur followed by a
pop when cur was a leaf, which leaves either `leaf < 0` or `cur >= 0`.  (b) So at the top either cur is an
inner node, and the node phase visits it before its `break` is tested: one node consumed, at most three
(seven) pushed, all of them strict descendants; or cur is not an inner node and then, by (a) and the loop
condition, leaf < 0, and the leaf phase tests that leaf before its `break` is tested: one leaf consumed.
A threshold of 64 makes both `break`s unconditional, which only means one visit or one leaf per phase
instead of several.  (c) A finite tree has finitely many root-to-node paths; every trip retires one
stack entry or replaces it by entries of strictly deeper nodes, so the number of trips of one query is
bounded by the BVH4's nodes + leaves (under 40 000 for the largest tree here, the 20 000-triangle soup
with single-triangle leaves), far below the watchdog's 2^20.  A suspension (RES) leaves the loop between
two trips with the state saved whole and re-enters at the top: it adds no trip.  PRT_GUARD_TRIPS is left
alone and check_faults() is asserted clean after every launch: this file never trips the watchdog.

Part B creates each scene under each builder setting (tests/global_cases.py; what each setting does to
the tree is asserted on the CPU in tests/test_global_invariance.py) and compares hits and traced paths
with brute force, whose answers do not depend on the tree.  The fat-leaf scene puts leaves of 6, 7 and 8
triangles through the global kernel's leaf loop, the OCT leaf loop of the LDS kernels at both tree widths
and the pooled kernel's shadow traversal.
"""
import os

import numpy as np
import pytest

import global_cases as G
from kernel_parity import (T_MAX, T_MIN, OracleRefs, all_tiles, check_trace, hits_wrong, is_mis, nee_mode, open_scenes,
                           packed_camera, random_bounds, render_twice, variant_flags)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NTHREADS = min(16, len(os.sched_getaffinity(0)))
FACTOR = 4                     # work items per resident lane, at least: un-exhausted for most of the launch
GLOBAL_VARIANTS = (3, 5)       # reference estimator, MIS estimator
LDS_VARIANTS = (1, 2, 6, 7, 8)
DEPTH = 4
TILE = 64
REFS = OracleRefs()


@pytest.fixture(scope="module")
def scenes(cornell):
    """make(name, setting) -> DeviceScene of G.scene(name) created under G.knobs(setting) (cached)."""
    with open_scenes() as make:
        yield lambda name, setting: make(name, G.scene(cornell, name), **G.every_knob(setting))


def _tiles(W, H):
    return all_tiles(W, H, TILE)


# ================================================================== Part A: steady-state schedule
def _resident_lanes(ds):
    return ds.blocks_per_cu * ds.cus * 256


def _spp(ds, n_slots, at_least=1):
    """Samples per slot so that the launch has FACTOR items per resident lane."""
    return max(at_least, -(-FACTOR * _resident_lanes(ds) // n_slots))


def _frame_ref(cornell, name, mis, W, H, spp, depth, seed):
    """(slot sums, (extension, shadow) query counts) of the whole frame by the oracle's BVH2 backend on the
    library's default tree, computed once; that backend first has to equal BACKEND_BRUTE on sixteen 16 x 16
    tiles which include the frame's four corners (the oracle keys its draws by the global pixel, so the
    tile size does not matter)."""
    def compute():
        from pyrenderer_amd._native import Bvh
        flat = G.scene(cornell, name)
        osc = O.OracleScene.from_flat(flat)
        with G.knobs({}):
            nodes, _, order = Bvh(flat.tri_v).export()
        osc.set_bvh(nodes, order)
        cam = packed_camera(cornell)
        tx, ty = (W + 15) // 16, (H + 15) // 16
        sub = np.unique(np.r_[0, tx - 1, tx * (ty - 1), tx * ty - 1,
                              np.random.default_rng(seed).choice(tx * ty, 12, replace=False)]).astype(np.int32)
        assert sub.size >= 8
        kw = dict(seed=seed, nthreads=NTHREADS)
        with nee_mode(mis):
            ref, cnt = osc.render_tiles(cam, W, H, TILE, TILE, _tiles(W, H), spp, depth, backend=O.BACKEND_BVH,
                                        counters=True, **kw)
            brute = osc.render_tiles(cam, W, H, 16, 16, sub, spp, depth, backend=O.BACKEND_BRUTE, **kw)
            walked = osc.render_tiles(cam, W, H, 16, 16, sub, spp, depth, backend=O.BACKEND_BVH, **kw)
        assert np.array_equal(walked, brute), (name, mis)
        # ... and those tiles of the whole frame are the same pixels
        full = O.unpack_tiles(ref, W, H, TILE, TILE, _tiles(W, H))
        assert np.array_equal(O.unpack_tiles(brute, W, H, 16, 16, sub)[_mask(W, H, sub)], full[_mask(W, H, sub)])
        assert np.isfinite(ref).all() and ref.mean() > 0
        return ref, (int(cnt[2]), int(cnt[3]))
    return REFS.get(("frame", name, mis, W, H, spp, depth, seed), compute)


def _mask(W, H, sub):
    """[x][y] mask of the 16 x 16 tiles `sub` of a W x H frame."""
    tx = (W + 15) // 16
    m = np.zeros((W, H), bool)
    for t in sub:
        m[(t % tx) * 16:(t % tx) * 16 + 16, (t // tx) * 16:(t // tx) * 16 + 16] = True
    return m


TRIP_WORDS = ("PRT_DIAG_WAVE_INNER", "PRT_DIAG_WAVE_LEAF", "PRT_DIAG_LANE_INNER", "PRT_DIAG_LANE_LEAF")


def _render(ds, cam, W, H, spp, depth, seed, v):
    """One launch through forced variant `v` in the production and in the STATS build: dict(img, queries,
    iters, trips).  Asserts what every launch of this file has to satisfy: the launch takes the global
    kernel asked for and stays un-exhausted (FACTOR), no watchdog trip, no non-finite sample, and the
    STATS image equals the production one (render_twice asserts the last three)."""
    from pyrenderer_amd import _native as N
    ids = _tiles(W, H)
    n_items = len(ids) * TILE * TILE * spp
    info = ds.kernel_info(n_items, variant_flags(v))
    assert info["variant"] == v and not info["lds_scene"] and info["quantized"] and info["bvh_arity"] == 4, info
    assert n_items >= FACTOR * _resident_lanes(ds), (n_items, _resident_lanes(ds))
    r = render_twice(ds, cam, W, H, TILE, ids, spp, depth, seed, variant_flags(v))
    w = r["words"]
    return dict(img=r["img"], queries=r["queries"], iters=int(w[N.PRT_DIAG_WAVE_ITERS]),
                trips=tuple(int(w[getattr(N, k)]) for k in TRIP_WORDS), items_per_lane=n_items / _resident_lanes(ds))


FRAME_A = dict(W=512, H=512, depth=DEPTH, seed=3)
_runs = {}


def _run(scenes, cornell, name, v, sched, W, H, depth, seed):
    """The cached render of one (scene, variant, schedule, frame); spp from the baseline scene's occupancy,
    at least 8 (512 x 512 x 8 on an MI355X: 5.3 items per resident lane)."""
    base_ds = scenes(name, G.SCHEDULES[G.BASELINE])
    spp = _spp(base_ds, len(_tiles(W, H)) * TILE * TILE, at_least=8)
    key = (name, v, sched, W, H, depth, seed)
    if key not in _runs:
        _runs[key] = _render(scenes(name, G.SCHEDULES[sched]), packed_camera(cornell), W, H, spp, depth, seed, v)
        r = _runs[key]
        print(f"{name} variant {v} {sched} {W}x{H}x{spp} depth {depth}: {r['items_per_lane']:.2f} items per resident "
              f"lane, {r['queries'][0]} ext / {r['queries'][1]} shadow queries, wave iterations {r['iters']}, "
              f"wave/lane inner/leaf trips {r['trips']}")
    return _runs[key], spp


def _check_schedule(scenes, cornell, name, v, sched, W, H, depth, seed):
    base, spp = _run(scenes, cornell, name, v, G.BASELINE, W, H, depth, seed)
    ref, counted = _frame_ref(cornell, name, is_mis(v), W, H, spp, depth, seed)
    differ = int((base["img"] != ref).any(axis=-1).sum())
    assert differ == 0, (name, v, "baseline against the oracle", differ)
    assert base["queries"] == counted, (base["queries"], counted)
    got, _ = _run(scenes, cornell, name, v, sched, W, H, depth, seed)
    differ = int((got["img"] != base["img"]).any(axis=-1).sum())
    assert differ == 0, (name, v, sched, differ)
    assert got["queries"] == counted, (sched, got["queries"], counted)     # a resumed query is counted once
    return base, got


@pytest.mark.parametrize("sched", list(G.SCHEDULES))
@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
@pytest.mark.parametrize("name", G.SMALL_SCENES)
def test_schedule_in_steady_state(scenes, cornell, name, v, sched):
    """Each threshold alone and the corners, 512 x 512 x 8 at depth 4: the frame equals the never-suspending
    baseline's, which equals the oracle's whole frame; the query counts equal the oracle's; no fault, no
    non-finite sample (_render).  On the zoo the sphere loop runs once per query, after a suspended query
    completes: a second pass would not change a closest hit, but a shadow query's count would move."""
    _check_schedule(scenes, cornell, name, v, sched, **FRAME_A)


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
@pytest.mark.parametrize("name", G.SMALL_SCENES)
def test_the_thresholds_took_effect(scenes, cornell, name, v):
    """The paths ran (STATS build).  A suspended query comes round the persistent loop again, so the waves
    iterate more often at PRT_RESUME_MIN=64 than at 1, where nothing is suspended.  Between the extremes of
    leaf_break and of leaf_exit each lane meets its nodes and leaves in another order, culls with another
    `best`, and the inner / leaf trip counts move."""
    run = {s: _run(scenes, cornell, name, v, s, **FRAME_A)[0]
           for s in ("resume-1", "resume-64", "break-0", "break-64", "exit-0", "exit-64")}
    assert run["resume-64"]["iters"] > run["resume-1"]["iters"], (run["resume-64"]["iters"], run["resume-1"]["iters"])
    assert run["break-0"]["trips"] != run["break-64"]["trips"], run["break-0"]["trips"]
    assert run["exit-0"]["trips"] != run["exit-64"]["trips"], run["exit-0"]["trips"]


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
def test_corner_on_a_ragged_frame(scenes, cornell, v):
    """200 x 136 (no multiple of the tile: lanes that drew a slot outside the frame) at (64, 64, 64)."""
    _check_schedule(scenes, cornell, "soup-3000", v, G.CORNER, W=200, H=136, depth=DEPTH, seed=6)


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
def test_corner_at_depth_1(scenes, cornell, v):
    """Paths of one extension query and its shadow ray at (64, 64, 64)."""
    _check_schedule(scenes, cornell, "soup-3000", v, G.CORNER, W=512, H=512, depth=1, seed=5)


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
def test_corner_multi_frame_launch(scenes, cornell, v):
    """Three progressive frames (frame_stride = spp) through one persistent launch at (64, 64, 64): each
    frame equals the baseline scene's accumulate call for its samples, frame 0 the oracle's frame."""
    import torch
    cam = packed_camera(cornell)
    W = H = 256
    n, seed, name = 3, 7, "soup-3000"
    ids = _tiles(W, H)
    n_slots = len(ids) * TILE * TILE
    base_ds = scenes(name, G.SCHEDULES[G.BASELINE])
    spp = _spp(base_ds, n * n_slots)
    info = base_ds.kernel_info(n * n_slots * spp, variant_flags(v))
    assert info["variant"] == v and not info["lds_scene"], info
    assert n * n_slots * spp >= FACTOR * _resident_lanes(base_ds)
    frames = {}
    for sched in (G.BASELINE, G.CORNER):
        ds = scenes(name, G.SCHEDULES[sched])
        out = torch.full((n, n_slots * 3), float("nan"), dtype=torch.float32, device="cuda:0")
        ds.render_frames_device(cam, W, H, TILE, TILE, ids, spp, DEPTH, n, out.data_ptr(), None, seed=seed,
                                frame_stride=spp, flags=variant_flags(v))
        ds.check_faults()
        frames[sched] = out.cpu().numpy().reshape(n, n_slots, 3)
    ref, _ = _frame_ref(cornell, name, is_mis(v), W, H, spp, DEPTH, seed)
    assert np.array_equal(frames[G.BASELINE][0], ref)
    for f in range(n):
        acc = np.zeros((n_slots, 3), np.float32)
        base_ds.render_tiles_accumulate(cam, W, H, TILE, TILE, ids, f * spp, spp, DEPTH, acc, seed=seed,
                                        flags=variant_flags(v))
        for sched in frames:
            assert np.array_equal(frames[sched][f], acc), (sched, f)


# ================================================================== Part B: tree shapes
TREE_CASES = [(name, tree) for name in G.SCENES for tree in G.TREES if (name, tree) not in G.DROPPED]


def _osc(cornell, name):
    return REFS.get(("scene", name), lambda: O.OracleScene.from_flat(G.scene(cornell, name)))


def _oracle_hits(cornell, name, key):
    """Brute-force (id, t), shadow-style bounds and the bounded any-hit booleans of one ray set, once."""
    def compute():
        osc = _osc(cornell, name)
        o, d = G.ray_sets(cornell, name)[key]
        tmax = random_bounds(osc, o, d, 3)
        return REFS.closest((name, key), osc, o, d), tmax, osc.closest(o, d, T_MIN, tmax)[0] != 0
    return REFS.get(("hits", name, key), compute)


def _check_hits(ds, cornell, name, quantized):
    wrong = []
    for key, (o, d) in G.ray_sets(cornell, name).items():
        closest, tmax, ohit = _oracle_hits(cornell, name, key)
        n, first, _ = hits_wrong(ds, None, o, d, T_MIN, T_MAX, quantized, any_hit=False, want=closest)
        if n:
            wrong.append((key, "closest", n, first))
        n, first, _ = hits_wrong(ds, None, o, d, T_MIN, tmax, quantized, any_hit=True, want=ohit)
        if n:
            wrong.append((key, "any-hit", n, first))
        assert 0.2 < ohit.mean() < 0.8, (key, ohit.mean())               # the bounds do separate the rays
    ds.check_faults()
    assert not wrong, (name, [w[:3] for w in wrong], wrong)


def _check_trace(ds, cornell, name, v):
    for key, (o, d) in G.ray_sets(cornell, name).items():
        ref = REFS.trace((name, key), _osc(cornell, name), o, d, DEPTH, 17, is_mis(v), nthreads=NTHREADS)
        check_trace(ds, ref, o, d, DEPTH, 17, v, label="%s %s" % (name, key))


def _tree_scene(scenes, cornell, name, setting):
    """The device scene under one builder setting; its BVH2 is the tree the CPU file examined."""
    ds = scenes(name, setting)
    rep = G.tree_report(G.scene(cornell, name), setting)
    assert (ds.n_nodes, ds.bvh_depth) == (rep["bvh2_nodes"], rep["bvh2_depth"]), (name, setting)
    return ds


@pytest.mark.parametrize("quantized", [False, True])
@pytest.mark.parametrize("name,tree", TREE_CASES)
def test_hits_over_every_tree(scenes, cornell, name, tree, quantized):
    """prt_closest_hits, closest in (id, t) and bounded any-hit, on f32 and quantised nodes: the interior
    rays and seed 17's rays from 100 extents outside."""
    ds = _tree_scene(scenes, cornell, name, G.tree_setting(name, tree))
    assert not ds.kernel_info()["lds_scene"]
    _check_hits(ds, cornell, name, quantized)


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
@pytest.mark.parametrize("name,tree", TREE_CASES)
def test_paths_over_every_tree(scenes, cornell, name, tree, v):
    """prt_trace_rays, 4096 + 4096 caller rays at depth 4 through the global-scene kernels."""
    ds = _tree_scene(scenes, cornell, name, G.tree_setting(name, tree))
    info = ds.kernel_info(G.N_RAYS, variant_flags(v))
    assert info["variant"] == v and not info["lds_scene"] and info["bvh_arity"] == 4, info
    _check_trace(ds, cornell, name, v)


def test_large_scene_spills_its_stack(scenes, cornell):
    """The 20 000-triangle soup's BVH4 asks for more entries than the LDS part of the spill stack holds
    at the default PRT_SPILL_LDS, and a render's deepest entry does go past it (STATS, word 13)."""
    from pyrenderer_amd import _native as N
    ds = scenes("soup-20000", {})
    info = ds.kernel_info(256 * 256 * 8, variant_flags(N.VAR_GLOBAL))
    assert info["variant"] == N.VAR_GLOBAL and info["stack"] == 16, info
    ds.render_tiles(packed_camera(cornell), 256, 256, TILE, TILE, _tiles(256, 256), 8, 8, 1,
                    variant_flags(N.VAR_GLOBAL) | N.PRT_FLAG_STATS)
    ds.check_faults()
    deepest = int(ds.diag_words(N.PRT_DIAG_WORDS)[N.PRT_DIAG_MAX_STACK])
    need = G.tree_report(G.scene(cornell, "soup-20000"), {})["stack_need"]
    print(f"soup-20000: deepest stack entry {deepest}, LDS part {info['stack']}, bound {need}")
    assert info["stack"] < deepest <= need, (deepest, info, need)


# ------------------------------------------------------------------ fat leaves
@pytest.mark.parametrize("quantized", [False, True])
def test_fat_leaves_hits(scenes, cornell, quantized):
    ds = _tree_scene(scenes, cornell, G.FAT, G.FAT_SETTING)
    _check_hits(ds, cornell, G.FAT, quantized)


@pytest.mark.parametrize("v", GLOBAL_VARIANTS)
def test_fat_leaves_through_the_global_kernels(scenes, cornell, v):
    """Leaves of 6, 7 and 8 coincident triangles (ties on every hit of a stack: the lowest id wins, and the
    copies differ in material) through variants 3 and 5, forced: the scene is LDS-resident."""
    ds = _tree_scene(scenes, cornell, G.FAT, G.FAT_SETTING)
    info = ds.kernel_info(G.N_RAYS, variant_flags(v))
    assert info["variant"] == v and info["bvh_arity"] == 4, info
    _check_trace(ds, cornell, G.FAT, v)


@pytest.mark.parametrize("v", LDS_VARIANTS)
@pytest.mark.parametrize("width", [4, 8])
def test_fat_leaves_through_the_lds_kernels(scenes, cornell, width, v):
    """The same leaves through the OCT triangle loop of the phase-aligned kernels (1, 2, 6) and the pooled
    kernels (7, 8: their shadow traversal too), over the BVH4 and the BVH8 in LDS."""
    ds = _tree_scene(scenes, cornell, G.FAT, dict(G.FAT_SETTING, PRT_LDS_WIDTH=width))
    info = ds.kernel_info(G.N_RAYS, variant_flags(v))
    assert info["variant"] == v and info["bvh_arity"] == width and info["lds_scene"], (width, v, info)
    _check_trace(ds, cornell, G.FAT, v)

"""Scenes, scene-creation settings and ray sets of the global-scene kernel's invariance tests: shared by
tests/test_global_invariance.py (CPU: every builder setting does to these scenes' trees what its case
is for) and tests/test_gpu_global_invariance.py (GPU: schedule thresholds in steady state, and every tree
shape, against the oracle's brute-force backend).

The scenes are the project's own (kernel_parity.soup_scene, hard_scenes, hard_spheres); nothing here
knows about the code under test except the names of the environment knobs, which prt_scene_create and
the BVH builder read once per scene.  Pure NumPy."""
import numpy as np

import hard_scenes as HS
import hard_spheres as SP
from kernel_parity import env_knobs, rays, soup_scene

# ------------------------------------------------------------------ knobs
SCHEDULE_KNOBS = ("PRT_RESUME_MIN", "PRT_LEAF_BREAK", "PRT_LEAF_EXIT")
TREE_KNOBS = ("PRT_SBVH", "PRT_ESC_BETA", "PRT_SBVH_BUDGET", "PRT_TREELET", "PRT_SAH_BINS", "PRT_BVH4_DP",
              "PRT_DP_LEAF", "PRT_MAX_LEAF")
# everything else the builder and the scene read that would change the tree or the schedule under the tests
OTHER_KNOBS = ("PRT_SBVH_ALPHA", "PRT_SAH_CT", "PRT_LEAF_MIN", "PRT_DP_CT", "PRT_BVH_VERBOSE", "PRT_LDS_WIDTH",
               "PRT_SPILL_LDS", "PRT_GUARD_TRIPS", "PRT_POOL_RESUME_MIN", "PRT_CHUNK_BYTES")
ALL_KNOBS = SCHEDULE_KNOBS + TREE_KNOBS + OTHER_KNOBS


def every_knob(setting):
    """`setting` (name -> value) with every other knob of ALL_KNOBS as None, which env_knobs unsets."""
    assert set(setting) <= set(ALL_KNOBS), setting
    return {k: setting.get(k) for k in ALL_KNOBS}


def knobs(setting):
    """The environment with exactly the knobs of `setting` set and every other knob of ALL_KNOBS unset;
    restored on exit.  Scenes and trees read the environment when they are created."""
    return env_knobs(**every_knob(setting))


def _sched(rm=None, lb=None, le=None):
    s = {"PRT_RESUME_MIN": rm, "PRT_LEAF_BREAK": lb, "PRT_LEAF_EXIT": le}
    return {k: v for k, v in s.items() if v is not None}


# Part A.  The global kernel's defaults are resume_min 32, leaf_break 16, leaf_exit 24, so "resume-32",
# "break-16" and "exit-24" are three spellings of the default; each knob is moved alone, then the corners.
BASELINE = "resume-1"        # a wave of 64 never has fewer than 1 lane traversing: no query is suspended
SCHEDULES = {
    "resume-1": _sched(rm=1), "resume-32": _sched(rm=32), "resume-64": _sched(rm=64),
    "break-0": _sched(lb=0), "break-16": _sched(lb=16), "break-64": _sched(lb=64),
    "exit-0": _sched(le=0), "exit-24": _sched(le=24), "exit-64": _sched(le=64),
    "corner-64-64-64": _sched(rm=64, lb=64, le=64),
    "corner-0-0-1": _sched(rm=1, lb=0, le=0),
}
CORNER = "corner-64-64-64"

# Part B.  "treelet" is PRT_TREELET=3 on the small scenes (their default is 0) and 0 on the large one (3).
TREES = {
    "default": {}, "sbvh-0": {"PRT_SBVH": 0}, "esc-0": {"PRT_ESC_BETA": 0}, "esc-1": {"PRT_ESC_BETA": 1},
    "budget-2": {"PRT_SBVH_BUDGET": 2}, "treelet": None, "bins-2": {"PRT_SAH_BINS": 2},
    "greedy": {"PRT_BVH4_DP": 0}, "dp-leaf-4": {"PRT_DP_LEAF": 4}, "max-leaf-1": {"PRT_MAX_LEAF": 1},
    "max-leaf-8": {"PRT_MAX_LEAF": 8},
}
LARGE_MIN = 1 << 14          # triangles from which the builder takes its large regime (prt_bvh.cpp)
N_LARGE = 20000
SMALL_SCENES = ("soup-3000", "slivers-1e-5", "soup-zoo")
SCENES = SMALL_SCENES + ("soup-20000",)
FAT = "stack"                # the fat-leaf scene, under FAT_SETTING
FAT_SETTING = {"PRT_MAX_LEAF": 8}
# (first triangle of a Cornell quad, coincident copies of it): floor x 8, ceiling x 6, back wall x 7
FAT_COPIES = ((0, 8), (2, 6), (4, 7))
# (scene, tree) pairs whose setting builds the default tree byte for byte, so that the case would only
# repeat "default" (tests/test_global_invariance.py asserts both halves: these are identical, every
# other pair differs).  PRT_MAX_LEAF=8 changes nothing without coincident geometry: the SAH never prefers
# a leaf of more than four of these triangles (the fat-leaf scene is where it does); the spatial-split
# budget does not bind on the two scenes whose splits end below 1.3 x; early split clipping at the small
# scenes' 64 x finds no triangle to clip in the zoo's 300-triangle soup.
DROPPED = frozenset([(s, "max-leaf-8") for s in SCENES] + [("soup-3000", "budget-2"), ("slivers-1e-5", "budget-2"),
                                                            ("soup-zoo", "esc-0")])


def tree_setting(scene, tree):
    if tree == "treelet":
        return {"PRT_TREELET": 0 if scene == "soup-20000" else 3}
    return TREES[tree]


def max_leaf_of(setting):
    return int(setting.get("PRT_MAX_LEAF", 4))


# ------------------------------------------------------------------ scenes
_scenes = {}


def stack(cornell_flat, copies=FAT_COPIES, seed=0):
    """The Cornell box with each quad of `copies` (first triangle -> number of coincident quads) that many
    times at the identical position, as hard_scenes.layers stacks the floor: successive copies carry
    different materials, one copy of each stack is an emitter that is also a light, and the index order is
    shuffled, so the lowest id of a tie is not the first copy.  No split separates identical boxes: where
    leaves of up to eight triangles are allowed the builder ends on leaves of exactly the stacks' heights,
    where only four are it cuts each stack by index.  Without fillers the scene stays LDS-resident at
    either tree width."""
    f = cornell_flat
    emitter = f.mat.shape[0]
    mat = np.concatenate([f.mat, np.array([[0.3, 0.6, 0.9, 1, 1, 1, 1, 0]], HS.F)])
    copy_mats = [3, 4, emitter, 5, 6, 3, 4]
    tv, tn, tm, lights = [f.tri_v], [f.tri_n], [f.tri_mat], HS._lights(f)
    n = f.n_tri
    for first, height in copies:
        for k in range(height - 1):
            tv.append(f.tri_v[first:first + 2])
            tn.append(f.tri_n[first:first + 2])
            tm.append(np.full(2, copy_mats[k % len(copy_mats)], np.int32))
            if copy_mats[k % len(copy_mats)] == emitter:
                lights = lights + [np.array([n, n + 1])]
            n += 2
    whole = HS._per_triangle(np.concatenate(tv), np.concatenate(tn), np.concatenate(tm), mat, lights, f.direct_rgb)
    return HS.reindexed(whole, np.random.default_rng(2000 + seed).permutation(whole.n_tri))


def scene(cornell, name):
    """The FlatScene of one name, built once per process and not modified by its users."""
    if name not in _scenes:
        if name == "soup-3000":
            flat = soup_scene(cornell, 3000, 9)
        elif name == "soup-20000":
            flat = soup_scene(cornell, N_LARGE, 9)
        elif name == "slivers-1e-5":
            flat = HS.case(cornell, name)[0]
        elif name == "soup-zoo":
            flat = SP.case(cornell, name)[0]
        elif name == FAT:
            flat = stack(cornell[2])
        else:
            raise KeyError(name)
        _scenes[name] = flat
    return _scenes[name]


# ------------------------------------------------------------------ rays
N_RAYS = 4096
FAR_SEED, FAR_EXTENTS = 17, 100.0
_ray_sets = {}


def ray_sets(cornell, name):
    """{"interior": (o, d), "far100": (o, d)}, N_RAYS rays each.  Interior: rays from inside the box (the
    sliver scene: 2048 aimed at its needles and 2048 random ones; the zoo: 2048 random ones and 2048 from
    inside its spheres); far100: seed 17's rays from 100 scene extents outside, aimed at the scene."""
    if name not in _ray_sets:
        flat = scene(cornell, name)
        if name == "slivers-1e-5":
            o, d = HS.case(cornell, name)[1]["aimed+random"]
            pick = np.r_[0:N_RAYS // 2, 4096:4096 + N_RAYS // 2]
            inner = (o[pick], d[pick])
        elif name == "soup-zoo":
            sets = SP.case(cornell, name)[1]
            inner = tuple(np.concatenate([sets["interior"][k][:N_RAYS // 2], sets["inside"][k][:N_RAYS // 2]])
                          for k in range(2))
        else:
            inner = rays(N_RAYS, 23)
        _ray_sets[name] = {"interior": inner, "far100": HS.far_rays(flat, N_RAYS, FAR_SEED, FAR_EXTENTS)[:2]}
    return _ray_sets[name]


# ------------------------------------------------------------------ trees on the host
def leaf_sizes(refs):
    """Triangle count of every leaf among child references (int32; a leaf is -(first * 8 + count - 1) - 1,
    an inner node >= 0, an empty slot of a wide node 0x7FFFFFFF)."""
    refs = np.asarray(refs, np.int32).ravel()
    v = -refs[refs < 0].astype(np.int64) - 1
    return (v & 7) + 1


def tree_report(flat, setting):
    """What the library builds of `flat` under `setting`: a dict of the BVH2's and the BVH4's integers, the
    leaf-size histograms of both (index = triangles per leaf, 0..8) and the BVH2 node array."""
    from pyrenderer_amd._native import Bvh
    with knobs(setting):
        b = Bvh(flat.tri_v, max_leaf=max_leaf_of(setting))
        nodes2, _, order = b.export()
        nodes4, depth4, need4 = b.collapse(4)
    refs2 = nodes2[:, 12:14].view(np.int32)
    refs4 = nodes4[:, 24:28].view(np.int32)
    return dict(triangles=flat.n_tri, references=b.n_tri, bvh2_nodes=b.n_nodes, bvh2_depth=b.depth,
                leaves=b.n_leaves, bvh4_nodes=nodes4.shape[0], bvh4_depth=depth4, stack_need=need4,
                leaf_hist2=np.bincount(leaf_sizes(refs2), minlength=9),
                leaf_hist4=np.bincount(leaf_sizes(refs4), minlength=9),
                nodes2=nodes2, nodes4=nodes4, order=order)


def same_tree(a, b):
    """Two tree_report results describe byte-identical BVH2 and BVH4 node arrays and the same order."""
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in ("nodes2", "nodes4", "order"))

"""The cases of tests/test_gpu_global_invariance.py against the host builder alone (no GPU): each
builder setting does to each scene's tree what its case is for, so the GPU file cannot pass on the
default tree eleven times over, and the fat-leaf scene does hold leaves of more than four triangles.
The trees come from the library's own builder (_native.Bvh under the same environment a scene is
created under; the GPU file asserts that the device scene reports the same BVH2).

Each count is a floor (or ceiling) well away from the value measured, which is quoted beside it.
"""
import numpy as np
import pytest

import global_cases as G
from hard_scenes import T_MAX, T_MIN, random_bounds
from oracle import oracle as O

_reports = {}


def _report(cornell, name, tree):
    setting = tree if isinstance(tree, dict) else G.tree_setting(name, tree)
    key = (name, tuple(sorted(setting.items())))
    if key not in _reports:
        _reports[key] = G.tree_report(G.scene(cornell, name), setting)
    return _reports[key]


def test_the_schedule_table_moves_each_knob_alone_and_the_corners():
    for knob, values in zip(G.SCHEDULE_KNOBS, ((1, 32, 64), (0, 16, 64), (0, 24, 64))):
        alone = sorted(s[knob] for s in G.SCHEDULES.values() if list(s) == [knob])
        assert alone == list(values), (knob, alone)
    assert G.SCHEDULES[G.CORNER] == {"PRT_RESUME_MIN": 64, "PRT_LEAF_BREAK": 64, "PRT_LEAF_EXIT": 64}
    assert G.SCHEDULES["corner-0-0-1"] == {"PRT_RESUME_MIN": 1, "PRT_LEAF_BREAK": 0, "PRT_LEAF_EXIT": 0}
    assert G.SCHEDULES[G.BASELINE] == {"PRT_RESUME_MIN": 1}


def test_knobs_are_set_and_restored(monkeypatch):
    import os
    monkeypatch.setenv("PRT_SBVH", "7")
    monkeypatch.delenv("PRT_TREELET", raising=False)
    with G.knobs({"PRT_TREELET": 3}):
        assert os.environ["PRT_TREELET"] == "3" and "PRT_SBVH" not in os.environ
    assert os.environ["PRT_SBVH"] == "7" and "PRT_TREELET" not in os.environ


@pytest.mark.parametrize("name", G.SCENES)
def test_default_trees_hold_split_references(cornell, name):
    """More references than triangles under the default knobs; with spatial splits and early split clipping
    both off, one reference per triangle: PRT_SBVH=0 leaves only the clipped references."""
    n = G.scene(cornell, name).n_tri
    default, no_sbvh = _report(cornell, name, "default"), _report(cornell, name, "sbvh-0")
    neither = _report(cornell, name, {"PRT_SBVH": 0, "PRT_ESC_BETA": 0})
    esc_only = no_sbvh["references"] - n
    print(f"{name}: {n} triangles, {default['references']} references, {no_sbvh['references']} without spatial splits")
    assert default["references"] >= 1.1 * n             # measured 1.24 (soup-3000), 1.22, 1.30, 1.30
    assert neither["references"] == n
    assert 0 <= esc_only <= 40                          # measured 20, 1, 0, 20: the box's large triangles
    assert default["references"] - no_sbvh["references"] >= 0.1 * n           # measured 0.23, 0.20, 0.30, 0.30


@pytest.mark.parametrize("name", G.SCENES)
def test_esc_beta_1_clips_many_references(cornell, name):
    """PRT_ESC_BETA=1 clips every triangle above the mean box area; 0 clips none."""
    many, none = _report(cornell, name, "esc-1"), _report(cornell, name, "esc-0")
    print(f"{name}: {many['references']} references at beta 1, {none['references']} at 0")
    assert many["references"] >= 1.1 * none["references"]      # measured 1.29, 1.72, 1.38, 1.20


@pytest.mark.parametrize("tree", ["greedy", "dp-leaf-4"])
@pytest.mark.parametrize("name", G.SCENES)
def test_collapse_knobs_change_the_bvh4_alone(cornell, name, tree):
    """PRT_BVH4_DP=0 and PRT_DP_LEAF=4 leave the BVH2 alone and collapse it into another BVH4: more nodes
    greedily (measured +15 %, +7 %, +13 %, +16 %), fewer with merged leaves (-15 %, -25 %, -11 %, -16 %), which
    then hold three and four triangles."""
    default, got = _report(cornell, name, "default"), _report(cornell, name, tree)
    assert got["nodes2"].tobytes() == default["nodes2"].tobytes()
    if tree == "greedy":
        assert got["bvh4_nodes"] > default["bvh4_nodes"], (got["bvh4_nodes"], default["bvh4_nodes"])
    else:
        assert got["bvh4_nodes"] <= 0.95 * default["bvh4_nodes"], (got["bvh4_nodes"], default["bvh4_nodes"])
        assert got["leaf_hist4"][3:5].sum() > default["leaf_hist4"][3:5].sum() and got["leaf_hist4"][4] >= 1
        assert got["leaf_hist4"][5:].sum() == 0


@pytest.mark.parametrize("name", G.SCENES)
def test_max_leaf_1_makes_single_triangle_leaves(cornell, name):
    rep = _report(cornell, name, "max-leaf-1")
    assert rep["leaf_hist2"][1] == rep["leaves"] == rep["references"] and rep["leaf_hist2"][2:].sum() == 0
    assert rep["leaf_hist4"][1] == rep["references"] and rep["leaf_hist4"][2:].sum() == 0
    assert _report(cornell, name, "default")["leaf_hist2"][2] >= 0.4 * _report(cornell, name, "default")["leaves"]


@pytest.mark.parametrize("name", G.SCENES)
def test_treelet_and_bins_change_the_bvh2(cornell, name):
    """Treelet restructuring (3 passes on the small scenes, none on the large one) and two SAH bins build
    another BVH2 over the same references."""
    default = _report(cornell, name, "default")
    for tree in ("treelet", "bins-2"):
        got = _report(cornell, name, tree)
        assert got["nodes2"].tobytes() != default["nodes2"].tobytes(), tree
    assert _report(cornell, name, "treelet")["references"] == default["references"]


def test_every_kept_case_builds_another_tree_and_every_dropped_one_the_default(cornell):
    for name in G.SCENES:
        default = _report(cornell, name, "default")
        for tree in G.TREES:
            if tree == "default":
                continue
            same = G.same_tree(_report(cornell, name, tree), default)
            assert same == ((name, tree) in G.DROPPED), (name, tree, same)


def test_large_soup_takes_the_large_regime(cornell):
    """From 2^14 triangles on the builder uses 64 bins, early split clipping at 128 x and three treelet
    passes: the default tree of the 20 000-triangle soup is the one those values give and not the one the
    small scenes' values (32, 64 x, 0) give; for the 3000-triangle soup it is the other way round."""
    large = {"PRT_SAH_BINS": 64, "PRT_ESC_BETA": 128, "PRT_TREELET": 3}
    small = {"PRT_SAH_BINS": 32, "PRT_ESC_BETA": 64, "PRT_TREELET": 0}
    assert G.scene(cornell, "soup-3000").n_tri < G.LARGE_MIN <= G.scene(cornell, "soup-20000").n_tri
    for name, own, other in (("soup-20000", large, small), ("soup-3000", small, large)):
        default = _report(cornell, name, "default")
        assert G.same_tree(_report(cornell, name, own), default), name
        assert not G.same_tree(_report(cornell, name, other), default), name


def test_spill_area_is_live(cornell):
    """The BVH4's worst-case stack exceeds the 16 LDS entries of the default PRT_SPILL_LDS."""
    need = {name: _report(cornell, name, "default")["stack_need"] for name in G.SCENES}
    print("stack_need:", need)
    assert need["soup-3000"] >= 20 and need["soup-20000"] >= 28, need      # measured 25 and 34 (16, 19 on the others)


def test_fat_leaf_scene_has_leaves_of_six_seven_and_eight(cornell):
    """Under PRT_MAX_LEAF=8 each stack of coincident triangles ends in one leaf of its height, in the BVH2 and
    in the BVH4 the kernels walk; under the default of four there is no leaf above four.  The scene is small
    enough for the LDS-resident kernels at either width (the GPU file asserts the residency itself)."""
    flat = G.scene(cornell, G.FAT)
    fat, thin = _report(cornell, G.FAT, G.FAT_SETTING), _report(cornell, G.FAT, {})
    print(f"{G.FAT}: {flat.n_tri} triangles, leaf sizes {fat['leaf_hist2'].tolist()} (max_leaf 8), "
          f"{thin['leaf_hist2'].tolist()} (max_leaf 4)")
    for hist in (fat["leaf_hist2"], fat["leaf_hist4"]):
        assert hist[5:].sum() >= 3 and hist[8] >= 1          # measured: two leaves each of 6, 7 and 8
        assert [int(h) for h in hist[6:9]] == [2, 2, 2]      # one per triangle of each stacked quad
    assert thin["leaf_hist2"][5:].sum() == 0 and thin["leaf_hist4"][5:].sum() == 0
    assert fat["references"] == flat.n_tri == 36 + 2 * sum(h - 1 for _, h in G.FAT_COPIES)
    # the stacks are exact copies with differing materials, and the shuffle moved the lowest id off the original
    v = flat.tri_v.reshape(-1, 9)
    _, inverse, counts = np.unique(v, axis=0, return_inverse=True, return_counts=True)
    assert sorted(counts[counts > 1].tolist()) == [6, 6, 7, 7, 8, 8]
    for g in np.nonzero(counts > 1)[0]:
        assert len(set(flat.tri_mat[inverse.ravel() == g].tolist())) >= 4


def test_chain_scene_builds_no_fat_leaf(cornell):
    """bvh8_scenes.chain under PRT_MAX_LEAF=8: the SAH still peels the growing triangles off in ones and twos
    (no leaf above two), so it is not a fat-leaf scene and the GPU file does not use it as one."""
    import bvh8_scenes as S8
    rep = G.tree_report(S8.chain(cornell[2]), {"PRT_MAX_LEAF": 8})
    assert rep["leaf_hist2"][3:].sum() == 0 and rep["leaf_hist4"][3:].sum() == 0, rep["leaf_hist2"]


@pytest.mark.parametrize("name", G.SCENES + (G.FAT,))
def test_ray_sets_hit_and_their_bounds_separate(cornell, name):
    """Both ray sets of every scene end on geometry, the far set from outside the scene's box, and the
    shadow-style bounds leave between a fifth and four fifths of the rays occluded."""
    flat = G.scene(cornell, name)
    osc = O.OracleScene.from_flat(flat)
    v = flat.tri_v.reshape(-1, 3)
    for key, (o, d) in G.ray_sets(cornell, name).items():
        assert o.shape == d.shape == (G.N_RAYS, 3) and np.isfinite(o).all() and np.isfinite(d).all()
        hit = osc.closest(o, d, T_MIN, T_MAX)[0] != 0
        assert hit.mean() >= 0.45, (name, key, hit.mean())       # measured >= 0.57 (slivers, far: the open front)
        occluded = osc.closest(o, d, T_MIN, random_bounds(osc, o, d, 3))[0] != 0
        assert 0.2 < occluded.mean() < 0.8, (name, key, occluded.mean())
        if key == "far100":
            outside = ((o < v.min(0)) | (o > v.max(0))).any(axis=1)
            assert outside.all()

"""The eight-wide collapse of LDS-resident scenes' BVH2 (prt_bvh4.cpp collapse_bvh8, exported by
prt_bvh_collapse): the tree is a valid one — every triangle slot in exactly one leaf, every child box
around its subtree, at most eight children per node — its stack bound covers the deepest stack the
kernels' visits can reach, and asking for it leaves the BVH4 as it was.  CPU only."""
import json
import os

import numpy as np
import pytest

import bvh8_scenes as S8
import hard_scenes as HS
from conftest import GOLDEN, ROOT

EMPTY = 0x7FFFFFFF


def _specular_tri_v():
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.io_utils.read_tungsten import process_primitives
    d = json.load(open(os.path.join(ROOT, "pyrenderer_amd", "media", "cornell-box", "scene_specular.json")))
    scene, _ = process_primitives(d)
    return flatten_scene(scene).tri_v


def _tri_v(name, cornell):
    flat = cornell[2]
    if name in HOSTILE:
        return HS.case(cornell, name)[0].tri_v
    return {"cornell": lambda: flat.tri_v, "specular": _specular_tri_v,
            "five": lambda: S8.five_triangles(flat).tri_v, "nine-leaves": lambda: S8.nine_leaves(flat).tri_v,
            "soup": S8.soup, "lattice-small": lambda: HS.lattice_small(2)[0].tri_v,
            "soup-scene": lambda: S8.soup_scene(flat).tri_v}[name]()


# of tests/hard_scenes.py: coincident quads, needles, point and collinear triangles, a triangle referenced
# from several leaves, exact lattices, placements at other scales (two of them not LDS-resident: the
# collapse itself does not ask)
HOSTILE = ["layers-0", "layers-1", "layers-2", "slivers8-1e-5", "slivers-1e-5", "slivers-1e-3", "lattice-z", "box-p0",
           "box-p3", "soup-p3"]
SCENES = ["cornell", "specular", "five", "nine-leaves", "soup"] + HOSTILE + ["lattice-small", "soup-scene"]


@pytest.fixture(scope="module")
def trees(cornell):
    """name -> (Bvh, BVH2 nodes, {width: (children per node, depth, stack_need)}); children = list of
    (lo[3], hi[3], ref) of the non-empty slots, after checking that the empty ones are the last."""
    from pyrenderer_amd import _native as N
    made = {}

    def get(name):
        if name not in made:
            b = N.Bvh(np.ascontiguousarray(_tri_v(name, cornell), np.float32).reshape(-1, 9), max_leaf=4)
            made[name] = (b, b.export()[0], {w: _children(b, w) for w in (8, 4)})
        return made[name]
    return get


def _children(b, width):
    nodes, depth, need = b.collapse(width)
    assert nodes.shape[1] == (32 if width == 4 else 56)
    out = []
    for nd in nodes:
        refs = nd[6 * width:7 * width].view(np.int32)
        ch = []
        for k in range(width):
            p = nd[(k // 4) * 24 + k % 4:(k // 4) * 24 + 24:4]   # lo.x hi.x lo.y hi.y lo.z hi.z
            lo, hi = p[0::2], p[1::2]
            if refs[k] == EMPTY:
                assert np.all(lo == np.inf) and np.all(hi == -np.inf)
            else:
                assert len(ch) == k, "a child after an empty slot"
                ch.append((lo.copy(), hi.copy(), int(refs[k])))
        out.append(ch)
    return out, depth, need


def _leaf_slots(ref):
    v = -ref - 1
    return range(v >> 3, (v >> 3) + (v & 7) + 1)


def _bvh2_leaf_boxes(nodes2):
    """slot -> (lo, hi) of the BVH2 leaf that holds it."""
    boxes = {}
    for nd in nodes2:
        for side in (0, 1):
            ref = int(nd[12 + side:13 + side].view(np.int32)[0])
            bx = nd[6 * side:6 * side + 6]
            if ref < 0 and bx[0] <= bx[1]:
                for s in _leaf_slots(ref):
                    boxes[s] = (bx[0::2], bx[1::2])
    return boxes


@pytest.mark.parametrize("name", SCENES)
def test_bvh8_is_a_valid_tree(trees, name):
    b, nodes2, by_width = trees(name)
    tree, depth, _ = by_width[8]
    leaf_box = _bvh2_leaf_boxes(nodes2)
    seen = np.zeros(b.n_tri, np.int32)     # references in BVH order
    visited = np.zeros(len(tree), np.int32)

    def slots_under(ref):
        if ref < 0:
            return list(_leaf_slots(ref))
        return [s for _, _, r in tree[ref] for s in slots_under(r)]

    deepest, stack = 0, [(0, 0)]
    while stack:
        i, d = stack.pop()
        visited[i] += 1
        deepest = max(deepest, d)
        assert 1 <= len(tree[i]) <= 8
        for lo, hi, ref in tree[i]:
            under = slots_under(ref)
            for s in under:
                blo, bhi = leaf_box[s]
                assert np.all(lo <= blo) and np.all(bhi <= hi), (name, i, ref, s)
            if ref < 0:
                seen[list(_leaf_slots(ref))] += 1
            else:
                stack.append((ref, d + 1))
    assert (seen == 1).all() and (visited == 1).all()
    assert depth == deepest
    if name == "five":
        assert len(tree) == 1 and all(r < 0 for _, _, r in tree[0])
    if name == "nine-leaves":
        assert b.n_leaves == 9 and len(tree) == 2
    if name == "cornell":
        assert len(tree) == 3 and len(by_width[4][0]) == 7


def _deepest_stack(tree, width):
    """Entries of the deepest stack a traversal reaches when every child of every node is hit: index 0 holds
    the sentinel, a visit entered with its top at index sp writes its pushes above it without a branch
    (closest-hit: children width-1 .. 1, advancing for all but the first; any-hit: children 0 .. width-2,
    advancing for each hit) and whichever child it continues with is entered above the others."""
    worst, stack = 0, [(0, 0)]
    while stack:
        i, sp = stack.pop()
        c = len(tree[i])
        for order, pushed in ((range(width - 1, 0, -1), lambda k: k < c), (range(width - 1), lambda k: k < c)):
            top = sp
            for k in order:
                worst = max(worst, top + 1 + 1)   # the slot written, as a count of entries
                top += 1 if pushed(k) else 0
        for _, _, ref in tree[i]:
            if ref >= 0:
                stack.append((ref, sp + c - 1))
    return worst


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("width", [4, 8])
def test_stack_need_covers_the_worst_case_traversal(trees, name, width):
    tree, _, need = trees(name)[2][width]
    reach = _deepest_stack(tree, width)
    assert need >= reach, (name, width, need, reach)
    assert need <= reach + width - 1          # and is no idle bound


@pytest.mark.parametrize("name", SCENES)
def test_bvh4_is_unchanged_by_the_width_option(trees, name, cornell):
    from pyrenderer_amd import _native as N
    from kernel_parity import fnv1a64
    b = trees(name)[0]
    fresh = N.Bvh(np.ascontiguousarray(_tri_v(name, cornell), np.float32).reshape(-1, 9), max_leaf=4)
    first = fresh.collapse(4)            # before this handle was ever asked for the eight-wide tree
    fresh.collapse(8)
    for got in (fresh.collapse(4), b.collapse(4)):
        assert np.array_equal(got[0].view(np.uint32), first[0].view(np.uint32)) and got[1:] == first[1:]
    if name == "cornell":
        pinned = json.load(open(os.path.join(GOLDEN, "bvh_trees.json")))["cornell"]
        assert fnv1a64(first[0]) == pinned["nodes4"]
        assert (len(first[0]), first[1], first[2]) == (pinned["bvh4_nodes"], pinned["bvh4_depth"], pinned["stack_need"])


@pytest.mark.parametrize("name", ["layers-0", "slivers8-1e-5"])
def test_hostile_lds_scenes_have_a_two_level_bvh8(trees, name):
    """What tests/test_gpu_lds_width_hard.py relies on: forced to width 8, these scenes give the eight-wide
    kernels a tree with a second level of inner nodes and more stack than the Cornell box's 15 entries."""
    tree, depth, need = trees(name)[2][8]
    assert depth == 2 and 15 < need <= 32, (name, depth, need)
    assert any(r >= 0 for i in [r for _, _, r in tree[0] if r >= 0] for _, _, r in tree[i])


def test_chain_scene_needs_more_stack_at_width_8(cornell):
    """The scene tests/test_gpu_lds_bvh8.py uses for the width rule's stack limit."""
    from pyrenderer_amd import _native as N
    b = N.Bvh(S8.chain(cornell[2]).tri_v, max_leaf=S8.CHAIN_MAX_LEAF)
    assert b.collapse(4)[2] <= 32 < b.collapse(8)[2]


def test_collapse_rejects_other_widths():
    from pyrenderer_amd import _native as N
    b = N.Bvh(S8.soup(8), max_leaf=4)
    info = np.zeros(4, np.int64)
    assert N.lib().prt_bvh_collapse(b.h, 2, N.ptr(info), None) == -1
    assert N.lib().prt_bvh_collapse(b.h, 8, None, None) == -1

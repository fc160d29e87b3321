"""The device build's NumPy restatement (tests/lbvh_ref.py) on the CPU: on the test scenes and the
hostile shapes (no triangle, one, fewer than a leaf holds, equal centroids, one plane, duplicates) every
triangle sits in exactly one leaf of at most max_leaf slots, children are numbered above their parents and level
by level, the filled boxes contain their triangles and children, the stack need is what an explicit depth-first
walk can hold, and the trees are the pinned ones."""
import numpy as np
import pytest

import global_cases as G
import lbvh_ref as L
import refit_ref as R

MAX_LEAF = 4
# (triangles, four-wide nodes, stack need, depth) under the rule of include/prt.h: 10 bits per axis, max_leaf 4
PINNED = {"cornell": (36, 8, 11, 3), "soup-3000": (3036, 546, 21, 6), "slivers-1e-5": (93, 17, 12, 3),
          "soup-zoo": (336, 62, 16, 4), "duplicates": (300, 49, 13, 3)}
PINNED8 = {"cornell": (4, 18)}


EDGES = ("none", "one", "three", "duplicates", "same-centroid", "plane")
SCENES = ("cornell", "soup-3000", "slivers-1e-5", "soup-zoo")


def tri_v_of(cornell, name):
    if name in EDGES:
        return L.edge_case(cornell[2].tri_v, name)
    return (cornell[2] if name == "cornell" else G.scene(cornell, name)).tri_v.reshape(-1, 9)


@pytest.fixture(scope="module")
def rebuilt(cornell):
    made = {}

    def get(name):
        if name not in made:
            made[name] = (tri_v_of(cornell, name), L.rebuild(tri_v_of(cornell, name), MAX_LEAF))
        return made[name]
    return get


@pytest.mark.parametrize("name", SCENES + EDGES)
def test_tree_invariants(rebuilt, name):
    tri_v, t = rebuilt(name)
    n = tri_v.shape[0]
    assert sorted(t["order"].tolist()) == list(range(n))          # one slot per triangle
    codes = t["codes"][t["order"]]
    assert (np.diff(codes.astype(np.int64)) >= 0).all() and int(t["codes"].max(initial=0)) < 1 << 30
    same = np.diff(codes.astype(np.int64)) == 0
    assert (np.diff(t["order"])[same] > 0).all()                   # the sort is stable
    for width in (4, 8):
        nodes, off = t[f"nodes{width}"], t[f"off{width}"]
        assert nodes.shape[0] == off[-1] >= 1 and off[1] == 1
        assert L.leaf_cover(nodes, width, n, MAX_LEAF) == (0, 0), (name, width)
        assert L.numbering(nodes, width, off) == (0, 0, 0), (name, width)
        assert R.containment(nodes, width, t["order"], tri_v, t["pad"]) == (0, 0), (name, width)
        assert t[f"need{width}"] == L.walked_need(nodes, width), (name, width)
        assert t[f"depth{width}"] == len(off) - 2
        refs = R.refs_of(nodes, width)
        live = refs != R.EMPTY
        assert (live[:, :-1] >= live[:, 1:]).all()                 # empty slots stand after the children
        if n > MAX_LEAF:
            assert (live.sum(1) >= 2).all()
    assert t["nodes4q"].shape == (t["nodes4"].shape[0], 16)


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_trees(rebuilt, name):
    tri_v, t = rebuilt(name)
    assert (tri_v.shape[0], t["nodes4"].shape[0], t["need4"], t["depth4"]) == PINNED[name]
    if name in PINNED8:
        assert (t["nodes8"].shape[0], t["need8"]) == PINNED8[name]
    assert t["need4"] <= 32 and t["need8"] <= 32       # every stack variant stays testable on the test scenes


def test_small_roots(rebuilt):
    for name, count in (("none", 0), ("one", 1), ("three", 3)):
        t = rebuilt(name)[1]
        for width in (4, 8):
            nodes = t[f"nodes{width}"]
            refs = R.refs_of(nodes, width)
            assert nodes.shape[0] == 1 and t[f"need{width}"] == width and t[f"depth{width}"] == 0
            assert int((refs != R.EMPTY).sum()) == (1 if count else 0)
            if count:
                assert int(refs[0, 0]) == L.leaf_ref(0, count)
            assert np.isinf(nodes[0, R.plane(width - 1, 0)]) and nodes[0, R.plane(width - 1, 1)] == -np.inf


@pytest.mark.parametrize("name", ["duplicates", "same-centroid"])
def test_equal_codes_stay_balanced(rebuilt, name):
    """Equal codes split by position: the depth is that of a balanced tree, not the number of triangles."""
    tri_v, t = rebuilt(name)
    n = tri_v.shape[0]
    assert len(set(t["codes"].tolist())) == 1
    assert t["depth4"] <= int(np.ceil(np.log2(n) / 2)) and t["depth8"] <= int(np.ceil(np.log2(n) / 3))


def test_codes_follow_the_stated_rule(cornell):
    """A centroid on the upper bound lands in cell 1023, one on the lower in cell 0, an axis without extent in
    0; x is the most significant bit of each triple."""
    tri_v = L.grid(3)
    codes, c = L.morton_codes(tri_v)
    assert (codes & 0x09249249 == 0).all()                          # z: every centroid has the same
    top = np.argmax(c[:, 0] + c[:, 1])
    assert codes[top] >> 1 & 0x09249249 == 0x09249249 and codes[top] >> 2 & 0x09249249 == 0x09249249
    low = np.argmin(c[:, 0] + c[:, 1])
    assert codes[low] == 0
    x_only = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 0], [2, 0, 0, 3, 0, 0, 2, 0, 0]], np.float32)
    assert L.morton_codes(x_only)[0].tolist() == [0, 0x09249249 << 2]

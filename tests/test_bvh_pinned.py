"""The trees themselves, pinned.  Every other BVH test checks that a tree is valid (cover, nesting, one
leaf per slot, stack bound) or that images are bit-exact, and images are bit-exact for any valid tree:
a builder change that costs node visits passes them all.  Here the stand-alone driver
tools/sanitize/bvh_check.cpp (ASan + UBSan build of the builder units alone) prints FNV-1a-64 digests
of the five arrays a scene uploads — BVH2 nodes, triangle records, order, BVH4 nodes, quantised nodes —
and every integer statistic, and each case must equal its entry in tests/golden/bvh_trees.json.  The
trees are a function of the source, not of the optimiser (g++ -O1 and hipcc -O3 give the same bytes),
which the library cross-check below ties down: libprt.so's exported BVH2 hashes to the driver's digests.

An intended tree change regenerates the golden file:  python tests/test_bvh_pinned.py --regenerate
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tools", "sanitize")
OUT = os.path.join(ROOT, "build", "sanitize")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bvh_trees.json")
CORNELL_JSON = os.path.join(ROOT, "pyrenderer_amd", "media", "cornell-box", "scene.json")
REGENERATE = "python tests/test_bvh_pinned.py --regenerate"

KNOBS = ("PRT_SAH_BINS", "PRT_SBVH", "PRT_SBVH_ALPHA", "PRT_SBVH_BUDGET", "PRT_SAH_CT", "PRT_LEAF_MIN",
         "PRT_ESC_BETA", "PRT_TREELET", "PRT_BVH_VERBOSE", "PRT_BVH4_DP", "PRT_DP_CT", "PRT_DP_LEAF")
ARRAYS = ("nodes2", "tris", "order", "nodes4", "nodes4q")
INTEGERS = ("triangles", "references", "duplicates", "bvh2_nodes", "bvh2_depth", "leaves", "bvh4_nodes",
            "bvh4_depth", "stack_need", "spatial_splits", "sah_bits", "pad_bits")

R3K = ("--random", 3000, 3)
R20K = ("--random", 20000, 7, 8)
# id -> (driver arguments, knobs); "cornell" / "same50" name soups written by _soup()
CASES = {
    "random3000": (R3K, {}),
    "random3000_sbvh0": (R3K, {"PRT_SBVH": "0"}),
    "random3000_greedy": (R3K, {"PRT_BVH4_DP": "0"}),
    "random20000_leaf8": (R20K, {}),
    "random20000_leaf8_treelet0": (R20K, {"PRT_TREELET": "0"}),
    "cornell": (("cornell",), {}),
    "random9": (("--random", 9, 5), {}),
    "random0": (("--random", 0, 5), {}),
    "random1": (("--random", 1, 5), {}),
    "random2": (("--random", 2, 5), {}),
    "same50": (("same50", 4), {}),
    "random3000_leaf1": (R3K + (1,), {}),
    "random3000_leaf8": (R3K + (8,), {}),
    "random3000_dp_leaf4": (R3K, {"PRT_DP_LEAF": "4"}),
}


def _build():
    subprocess.run(["make", "-s", "-C", SAN, os.path.join(OUT, "bvh_check")], check=True, capture_output=True,
                   timeout=600)
    return os.path.join(OUT, "bvh_check")


def _cornell():
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    scene, _ = read_file(CORNELL_JSON)
    return np.ascontiguousarray(flatten_scene(scene).tri_v, np.float32).reshape(-1, 9)


def _soup(name, folder):
    """The named soup as a raw f32 file under `folder`."""
    path = os.path.join(str(folder), name + ".f32")
    if not os.path.exists(path):
        tv = _cornell() if name == "cornell" else np.tile(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32), (50, 1))
        tv.tofile(path)
    return path


def _run(exe, args, knobs, folder):
    args = [_soup(a, folder) if a in ("cornell", "same50") else str(a) for a in args]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def built():
    return _build()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tree_is_the_pinned_one(built, golden, case, tmp_path):
    args, knobs = CASES[case]
    got, want = _run(built, args, knobs, tmp_path), golden[case]
    assert got["failures"] == 0
    moved = [k for k in INTEGERS + ARRAYS if got[k] != want[k]]
    assert not moved, (f"{case}: {', '.join(moved)} differ from tests/golden/bvh_trees.json: "
                       f"{ {k: (got[k], want[k]) for k in moved} }.  The builder no longer produces the pinned "
                       f"tree; if the change of tree is intended, regenerate the file with `{REGENERATE}`.")


# ---------------------------------------------------------------- the library that ships builds the same trees

def _numpy_soup():
    rng = np.random.default_rng(29)
    n = 3000
    c = rng.uniform(-5, 5, (n, 1, 3))
    s = np.where(np.arange(n) % 40 == 0, 2.0, 0.15)[:, None, None]   # a few large triangles: split references
    return (c + rng.normal(0, 1, (n, 3, 3)) * s).astype(np.float32).reshape(n, 9)


@pytest.mark.parametrize("name", ["cornell", "numpy3000"])
def test_library_exports_the_drivers_tree(built, name, tmp_path, monkeypatch):
    """libprt.so (hipcc -O3) against the pinned g++ build: the same file, the same BVH2 bytes and info."""
    from kernel_parity import fnv1a64
    from pyrenderer_amd import _native as N
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    tv = _cornell() if name == "cornell" else _numpy_soup()
    path = tmp_path / (name + "_lib.f32")
    tv.tofile(path)
    rep = _run(built, (str(path), 4), {}, tmp_path)
    b = N.Bvh(tv, max_leaf=4)
    nodes, tris, order = b.export()
    assert (fnv1a64(nodes), fnv1a64(tris), fnv1a64(order)) == (rep["nodes2"], rep["tris"], rep["order"])
    assert (b.n_nodes, b.depth, b.n_leaves, b.n_tri) == (rep["bvh2_nodes"], rep["bvh2_depth"], rep["leaves"],
                                                         rep["references"])
    assert f"{np.array([b.pad], np.float32).view(np.uint32)[0]:08x}" == rep["pad_bits"]
    sah = np.array([int(rep["sah_bits"], 16)], np.uint64).view(np.float64)[0]
    assert round(b.sah_cost * 1000.0) == int(sah * 1000.0 + 0.5)


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit(f"usage: {REGENERATE}")
    import tempfile
    sys.path.insert(0, ROOT)
    exe = _build()
    with tempfile.TemporaryDirectory() as tmp:
        trees = {}
        for case_id, (case_args, case_knobs) in CASES.items():
            rep = _run(exe, case_args, case_knobs, tmp)
            trees[case_id] = {k: rep[k] for k in INTEGERS + ARRAYS}
    with open(GOLDEN, "w") as f:
        json.dump(trees, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(trees)} trees")

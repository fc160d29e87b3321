"""The refit's NumPy restatement (tests/refit_ref.py) against the host builder, on the CPU: with reference
splits off and unchanged geometry a bottom-up refit reproduces the collapsed trees byte for byte; under the
default knobs (references split at creation) it is never tighter than the build and still contains every
triangle and every child; and it stays so after a third of the triangles moved by half the scene's extent."""
import numpy as np
import pytest

import global_cases as G
import refit_ref as R

NO_SPLITS = {"PRT_SBVH": 0, "PRT_ESC_BETA": 0}
SCENES = ("cornell", "soup-3000")


def flat_of(cornell, name):
    return cornell[2] if name == "cornell" else G.scene(cornell, name)


def built(flat, setting):
    from pyrenderer_amd._native import Bvh
    with G.knobs(setting):
        b = Bvh(flat.tri_v)
        _, tris, order = b.export()
        return dict(pad=np.float32(b.pad), tris=tris, order=order, nodes4=b.collapse(4)[0], nodes8=b.collapse(8)[0])


@pytest.fixture(scope="module")
def trees(cornell):
    made = {}

    def get(name, setting_name):
        k = (name, setting_name)
        if k not in made:
            made[k] = built(flat_of(cornell, name), NO_SPLITS if setting_name == "no-splits" else {})
        return made[k]
    return get


@pytest.mark.parametrize("name", SCENES)
def test_unchanged_geometry_without_splits_is_the_built_tree(cornell, trees, name):
    flat, t = flat_of(cornell, name), trees(name, "no-splits")
    assert t["order"].size == flat.n_tri
    assert R.pad_rule(flat.tri_v).tobytes() == t["pad"].tobytes()
    got = R.refit(t["order"], t["nodes4"], t["nodes8"], flat.tri_v)
    for k in ("tris", "nodes4", "nodes8"):
        differ = int((got[k].view(np.uint32) != t[k].view(np.uint32)).sum())
        assert differ == 0, (name, k, differ)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("move", ["still", "moved"])
def test_default_knobs_stay_conservative(cornell, trees, name, move):
    flat, t = flat_of(cornell, name), trees(name, "default")
    if name == "soup-3000":
        assert t["order"].size > flat.n_tri     # references split at creation
    tri_v = flat.tri_v if move == "still" else R.displaced(flat.tri_v)
    got = R.refit(t["order"], t["nodes4"], t["nodes8"], tri_v)
    for width, key in ((4, "nodes4"), (8, "nodes8")):
        if move == "still":
            assert R.planes_outside(got[key], t[key], width) == 0, (name, width)
        assert R.containment(got[key], width, t["order"], tri_v, got["pad"]) == (0, 0), (name, width, move)


def test_quantiser_contains_the_float_boxes(cornell, trees):
    """The restated quantiser's boxes hold the f32 ones with the pad to spare (the pin against the library's own
    words is on the GPU, tests/test_gpu_refit.py)."""
    t = trees("soup-3000", "default")
    q = R.quantize4(t["nodes4"], t["pad"])
    qi = q.view(np.uint32)
    refs = R.refs_of(t["nodes4"], 4)
    live = refs != R.EMPTY
    assert (np.ascontiguousarray(qi[:, 12:16]).view(np.int32) == refs).all()
    for a in range(3):
        o, st = q[:, a].astype(np.float64)[:, None], q[:, 3 + a].astype(np.float64)[:, None]
        sh = 8 * np.arange(4)[None]
        lo = o + ((qi[:, 6 + 2 * a][:, None] >> sh) & 255) * st
        hi = o + ((qi[:, 7 + 2 * a][:, None] >> sh) & 255) * st
        assert (lo[live] <= t["nodes4"][:, 8 * a:8 * a + 4][live] - t["pad"]).all()
        assert (hi[live] >= t["nodes4"][:, 8 * a + 4:8 * a + 8][live] + t["pad"]).all()

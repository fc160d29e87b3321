"""The entry points of the temporal accumulation across moving objects and their front ends without a GPU:
declared, exported and bound under ABI 4; bad arguments rejected before any device is touched, with the
denoiser's own error text and the entry point's name in front; the Python ValueErrors; motion_rows, moved and
the --spin switch."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from temporal_abi_cases import FAKE, GOOD, MAX_OBJECTS, call, cam as _cam

NAMES = ("prt_temporal_accumulate_motion", "prt_temporal_accumulate_motion_device")


def test_header_and_exports_carry_the_entry_points():
    from pyrenderer_amd import _native as N
    src = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z_0-9]+)\s*\(", src))
    L = N.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in N.EXPORTS, n
        assert hasattr(L, n), n
    assert L.prt_abi_version() == 4 and "#define PRT_ABI_VERSION 4" in src
    # the contract stands beside the static one, with its finiteness statement
    block = src[src.index("Temporal accumulation across moving objects"):src.index("int prt_temporal_accumulate_motion(")]
    for word in ("no table entry is read", "no previous pose", "prev_ids[q] == ids[p]", "-0", "Finiteness", "1048576"):
        assert word in block, word
    # the device form takes one argument more than the host form, the stream
    assert len(N.EXPORTS[NAMES[1]][1]) == len(N.EXPORTS[NAMES[0]][1]) + 1 == 18


def test_the_kernel_lives_in_the_auxiliary_unit_only():
    import json
    from pyrenderer_amd import build as B
    homes = [f for f in B.SOURCES + B.HEADERS + [B.TRACE_INST] + B.AUX_SOURCES + B.AUX_HEADERS
             if re.search(r"\bstruct Motion\b|\btemporal_kernel<true>", open(os.path.join(B.CSRC, f)).read())]
    assert homes and set(homes) <= set(B.AUX_SOURCES + B.AUX_HEADERS), homes
    src = open(os.path.join(B.CSRC, "prt_denoise.hip")).read()
    assert "template <bool kMotion>" in src and "temporal_kernel<false>" in src and "temporal_kernel<true>" in src
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["prt_denoise.h"]
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
    assert B.kernel_sha() in json.dumps(pmc)


# every bad argument the motion entry points add, and a few of those they share with prt_temporal_accumulate
_CASES = [("null_ids", b"NULL"), ("null_color", b"NULL"), ("null_state", b"NULL"), ("null_params", b"params8"),
          ("only_prev_ids", b"NULL together"), ("no_prev_ids", b"NULL together"), ("no_prev_state", b"NULL together"),
          ("only_prev_state", b"NULL together"), ("n_neg", b"n_objects"), ("n_huge", b"n_objects"),
          ("null_motion", b"motion is NULL"), ("w0", b"W and H"), ("h_huge", b"W and H"), ("device_neg", b"device"),
          ("aperture", b"aperture"), ("tau_z", b"tau_z")]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _CASES)
def test_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    from pyrenderer_amd import _native as N
    rc, msg, who, state = call(N.lib(), N, device_form, case, motion=True)
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(who) and word in msg, msg
    assert (state == 1).all()


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case", ["legal", "legal_empty", "legal_first", "legal_max"])
def test_legal_calls_end_at_the_device_ordinal(case, device_form):
    """A legal call passes every argument check and ends at the device ordinal, which is asked for last: one that
    no machine has is "no such device", or "no HIP device" without a GPU.  Nothing runs either way."""
    from pyrenderer_amd import _native as N
    rc, msg, who, _ = call(N.lib(), N, device_form, case, motion=True)
    assert rc in (-1, -2) and msg.startswith(who) and (b"no such device" in msg or b"no HIP device" in msg), (rc, msg)


def test_device_form_checks_alignment_and_aliasing_without_a_gpu():
    from pyrenderer_amd import _native as N
    L = N.lib()
    par, cam, pcam = np.array(GOOD, np.float32), _cam(), _cam()
    pcam[3] = 0.25

    def dev(state=FAKE * 3, ids=FAKE * 6, pids=FAKE * 7, motion=FAKE * 8, out=None, var=None):
        rc = L.prt_temporal_accumulate_motion_device(0, FAKE, FAKE * 2, N.ptr(cam), FAKE * 4, N.ptr(pcam), FAKE * 5, ids,
                                                     pids, motion, 3, 70, 130, N.ptr(par), state, out, var, None)
        return rc, L.prt_denoise_last_error()

    rc, msg = dev(state=FAKE * 3 + 4)
    assert rc == -1 and msg.startswith(b"prt_temporal_accumulate_motion_device:") and b"aligned" in msg, msg
    for kw in (dict(ids=FAKE * 6 + 2), dict(pids=FAKE * 7 + 1), dict(motion=FAKE * 8 + 3)):
        rc, msg = dev(**kw)
        assert rc == -1 and b"4-byte aligned" in msg, (kw, msg)
    for kw in (dict(state=FAKE * 6), dict(state=FAKE * 7), dict(out=FAKE * 8), dict(var=FAKE * 6), dict(var=FAKE * 7),
               dict(out=FAKE * 5), dict(out=FAKE * 9, var=FAKE * 9)):
        rc, msg = dev(**kw)
        assert rc == -1 and msg.startswith(b"prt_temporal_accumulate_motion_device:") and b"alias" in msg, (kw, msg)


# ------------------------------------------------------------------ Python ----

def test_python_wrappers_raise():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd import denoise as D
    c, f, cam = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32), _cam()
    st, ids, rows = D.temporal_state(2, 2), np.zeros((2, 2), np.int32), np.tile(D.IDENTITY_ROW, (1, 1))
    assert D.IDENTITY_ROW.tobytes() == np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32).tobytes()
    assert D.MAX_OBJECTS == MAX_OBJECTS
    with pytest.raises(ValueError, match="ids need a motion table"):
        D.temporal_accumulate(c, f, cam, ids=ids)
    with pytest.raises(ValueError, match="needs the frame's ids"):
        D.temporal_accumulate(c, f, cam, motion=rows)
    with pytest.raises(ValueError, match=r"prev must be \(state, feat, cam, ids\)"):
        D.temporal_accumulate(c, f, cam, (st, f, cam), ids=ids, motion=rows)
    with pytest.raises(ValueError, match=r"prev must be \(state, feat, cam, ids\)"):
        D.temporal_accumulate(c, f, cam, (st, f, cam, ids))
    with pytest.raises(ValueError, match="ids must be"):
        D.temporal_accumulate(c, f, cam, ids=np.zeros((2, 3), np.int32), motion=rows)
    with pytest.raises(ValueError, match="prev's ids must be"):
        D.temporal_accumulate(c, f, cam, (st, f, cam, np.zeros((3, 2), np.int32)), ids=ids, motion=rows)
    with pytest.raises(ValueError, match=r"motion must be \(n_objects, 12\)"):
        D.temporal_accumulate(c, f, cam, ids=ids, motion=np.zeros((2, 16), np.float32))
    with pytest.raises(ValueError, match="aperture"):
        D.temporal_accumulate(c, f, cam, (st, f, _cam(0.2), ids), ids=ids, motion=rows)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_motion: tau_z"):
        D.temporal_accumulate(c, f, cam, ids=ids, motion=rows, tau_z=0.0)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_motion: w_min"):   # an empty table is legal
        D.temporal_accumulate(c, f, cam, (st, f, cam, ids), ids=ids, motion=np.zeros((0, 12), np.float32), w_min=np.nan)
    with pytest.raises(ValueError, match="need the frame's d_ids_ptr"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, d_motion_ptr=FAKE * 4, n_objects=1)
    with pytest.raises(ValueError, match="ids need a motion table"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, d_ids_ptr=FAKE * 4)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_motion_device: motion is NULL"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, d_ids_ptr=FAKE * 4, n_objects=2)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_motion_device: .*NULL together"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, d_ids_ptr=FAKE * 4, n_objects=0,
                                     d_prev_ids_ptr=FAKE * 5)
    # the defaults keep today's entry points
    sig = inspect.signature(D.temporal_accumulate).parameters
    assert sig["ids"].default is None and sig["motion"].default is None
    sig = inspect.signature(D.temporal_accumulate_device).parameters
    assert all(sig[k].default is None for k in ("d_ids_ptr", "d_prev_ids_ptr", "d_motion_ptr", "n_objects"))


@pytest.fixture(scope="module")
def cornell_scene():
    from pyrenderer_amd import scenes as S
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    return read_file(S.CORNELL)[0]


def _move():
    """A rotation about a tilted axis and a shift."""
    k = np.array([0.3, 0.9, -0.2])
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(25.0)
    G = np.eye(4)
    G[:3, :3] = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
    G[:3, 3] = (0.1, -0.05, 0.2)
    return G


def test_motion_rows_and_moved(cornell_scene):
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd import scenes as S
    from pyrenderer_amd.core.bsdf import BSDF
    from pyrenderer_amd.flatten import flatten_scene
    from pyrenderer_amd.mathematics.shapes import Cube, Quad, Sphere, TriangleMesh
    scene, G = cornell_scene, _move()
    assert isinstance(scene.primitives[5], Cube) and isinstance(scene.primitives[0], Quad)
    later = S.moved(scene, {5: G})
    # moved(): G applied to the old world vertices, everything else and every BSDF shared
    old, new = scene.primitives[5], later.primitives[5]
    assert np.abs(new.vertices - (old.vertices @ G[:3, :3].T + G[:3, 3])).max() <= 1e-12
    assert np.array_equal(new.faces, old.faces) and new.bsdf is old.bsdf and type(new) is Cube
    assert np.abs(new.normal_vectors - old.normal_vectors @ G[:3, :3].T.astype(np.float32)).max() <= 1e-6
    assert all(later.primitives[i] is scene.primitives[i] for i in range(8) if i != 5)
    assert later.lights == scene.lights and len(scene.primitives) == 8
    assert np.array_equal(flatten_scene(later).mat, flatten_scene(scene).mat)
    assert np.array_equal(flatten_scene(later).tri_mat, flatten_scene(scene).tri_mat)
    # motion_rows: `scene` is the earlier frame's here, so the row of the move back is G itself
    rows = D.motion_rows(later, scene)
    assert rows.shape == (8, 12) and rows.dtype == np.float32
    assert np.abs(rows[5].reshape(3, 4) - G[:3]).max() <= 1e-6
    for i in range(8):
        if i != 5:
            assert rows[i].tobytes() == D.IDENTITY_ROW.tobytes(), i
    back = D.motion_rows(scene, later)[5].reshape(3, 4)
    assert np.abs(back - np.linalg.inv(G)[:3]).max() <= 1e-6
    assert all(r.tobytes() == D.IDENTITY_ROW.tobytes() for r in D.motion_rows(scene, scene))
    # a scaled primitive has no rigid motion: a NaN row
    scaled = S.moved(scene, {})
    scaled.primitives[6] = Cube(np.diag([1.1, 1.0, 1.0, 1.0]) @ scene.primitives[6].trans_mat, scene.primitives[6].bsdf)
    rows = D.motion_rows(scene, scaled)
    assert np.isnan(rows[6]).all() and rows[5].tobytes() == D.IDENTITY_ROW.tobytes()
    mirrored = S.moved(scene, {})
    mirrored.primitives[6] = Cube(np.diag([-1.0, 1.0, 1.0, 1.0]) @ scene.primitives[6].trans_mat, scene.primitives[6].bsdf)
    assert np.isnan(D.motion_rows(scene, mirrored)[6]).all()
    # mismatched scenes
    short = S.moved(scene, {})
    short.primitives.pop()
    with pytest.raises(ValueError, match="same primitives in the same order"):
        D.motion_rows(scene, short)
    swapped = S.moved(scene, {})
    swapped.primitives[0], swapped.primitives[5] = swapped.primitives[5], swapped.primitives[0]
    with pytest.raises(ValueError, match="primitive 0 differs"):
        D.motion_rows(scene, swapped)
    other = S.moved(scene, {})
    other.primitives[5] = Cube(scene.primitives[5].trans_mat, scene.primitives[0].bsdf)   # another BSDF
    if not np.array_equal(scene.primitives[5].bsdf.pack(), scene.primitives[0].bsdf.pack()):
        with pytest.raises(ValueError, match="primitive 5 differs"):
            D.motion_rows(scene, other)
    # spheres move by their centre, a mesh keeps its faces and turns its explicit normals, a batch is rejected
    mat = BSDF({"type": "lambert", "albedo": [0.5, 0.5, 0.5]}).get_distribution()
    extra = S.moved(scene, {})
    extra.add_primitive(Sphere((0.1, 0.5, 0.2), 0.25, mat))
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    extra.add_primitive(TriangleMesh(np.eye(4), mat, v, np.array([[0, 1, 2]]), face_normals=np.array([[0, 0, 1]], np.float32)))
    pushed = S.moved(extra, {8: G, 9: G})
    assert np.allclose(pushed.primitives[8].center, G[:3, :3] @ extra.primitives[8].center + G[:3, 3])
    assert np.allclose(pushed.primitives[9].vertices, v @ G[:3, :3].T + G[:3, 3])
    assert np.allclose(pushed.primitives[9].normal_vectors[0], G[:3, 2], atol=1e-6)
    rows = D.motion_rows(extra, pushed)
    shift = extra.primitives[8].center - pushed.primitives[8].center
    assert np.allclose(rows[8].reshape(3, 4), np.concatenate([np.eye(3), shift[:, None]], 1), atol=1e-6)
    assert np.abs(rows[9].reshape(3, 4) - np.linalg.inv(G)[:3]).max() <= 1e-6
    grown = S.moved(extra, {})
    grown.primitives[8] = Sphere(extra.primitives[8].center, 0.3, mat)
    assert np.isnan(D.motion_rows(extra, grown)[8]).all()
    batch = S.moved(scene, {})
    batch.add_primitive(S.MeshBatch(v, np.array([[0, 1, 2]]), mat))
    with pytest.raises(ValueError, match="MeshBatch"):
        S.moved(batch, {8: G})
    assert D.motion_rows(batch, batch)[8].tobytes() == D.IDENTITY_ROW.tobytes()
    with pytest.raises(ValueError, match="not rigid"):
        S.moved(scene, {5: np.diag([2.0, 1.0, 1.0, 1.0])})
    with pytest.raises(ValueError, match="no primitive 8"):
        S.moved(scene, {8: G})
    # spun(): the same axis every frame, the first scene the scene itself
    seq = S.spun(scene, 5, 6.0, 3)
    assert seq[0] is scene and len(seq) == 3
    g = S.spin(scene.primitives[5], 6.0)
    assert np.abs(D.motion_rows(seq[1], seq[2])[5].reshape(3, 4) - np.linalg.inv(g)[:3]).max() <= 1e-6
    lo, hi = scene.primitives[5].bounding_box
    c = 0.5 * (np.asarray(lo) + np.asarray(hi))
    assert np.allclose(g[:3, :3] @ c + g[:3, 3], c) and np.allclose(g[1], (0, 1, 0, 0))


def test_the_accumulator_rejects_mismatched_scenes_before_it_renders(cornell_scene):
    from pyrenderer_amd import scenes as S
    from pyrenderer_amd.core.camera import Camera
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    cam = Camera((0, 1, 6.8), (0, 1, 0), (0, 1, 0), (8, 8), fov=20)
    short = S.moved(cornell_scene, {})
    short.primitives.pop(6)
    acc = TemporalAccumulator(cornell_scene, depth=2, spp=1)       # no device: the check comes first
    with pytest.raises(ValueError, match="same primitives in the same order"):
        acc.add(cam, short)
    with pytest.raises(ValueError, match="one scene per camera"):
        render_sequence(cornell_scene, [cam, cam], spp=1, depth=2, scenes=[cornell_scene])
    with pytest.raises(ValueError, match="add\\(camera\\) first"):
        acc.object_ids()
    assert inspect.signature(TemporalAccumulator.add).parameters["scene"].default is None
    assert inspect.signature(render_sequence).parameters["scenes"].default is None


# ------------------------------------------------------------ command line ----

def test_spin_flag():
    from pyrenderer_amd import main as M
    assert M.parse([]).spin is None
    a = M.parse(["--samples", "1", "--frames", "3", "--spin", "5", "6", "--temporal"])
    assert a.spin == (5, 6.0) and a.orbit == 0.0 and a.temporal
    a = M.parse(["--frames", "3", "--spin", "6", "-2.5", "--orbit", "1"])     # no history: every frame alone
    assert a.spin == (6, -2.5) and not a.temporal


@pytest.mark.parametrize("argv,flag", [
    (["--spin", "5", "6"], "--spin"),                                  # needs --frames
    (["--spin", "5", "6", "--temporal"], "--frames"),
    (["--frames", "3", "--spin", "x", "6"], "--spin"),
    (["--frames", "3", "--spin", "-1", "6"], "--spin"),
    (["--frames", "3", "--spin", "5", "nan"], "--spin"),
    (["--frames", "3", "--spin", "5"], "--spin"),
    (["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--spin", "5", "6"], "--spin"),
])
def test_spin_usage_errors(argv, flag, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.parse(argv)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err

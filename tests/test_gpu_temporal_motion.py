"""Temporal accumulation across moving objects on the GPU: prt_temporal_accumulate_motion against the NumPy
restatement (tests/temporal_ref.py with ids) bit for bit, the device entry point, the object-id plane, and a
Cornell box whose short box turns, end to end.

Measured on the MI355X for the end-to-end sequence below (Cornell 128^2, 1 spp, depth 8, the scene's static camera,
8 frames, the short box turned by 6 degrees and shifted by (0, 0, 0.02) per frame, default parameters): the share
of the box's hit pixels with history > 1 in frames 1..7 is 0.9818 0.9927 0.9680 0.9444 0.9768 0.9732 0.9776, least
0.9444 (SHARE); RMSE 0.012813 with the history against 0.051638 for the last frame alone, ratio 0.2481 (RHO_MOTION);
287 pixels uncovered by the box in frames 1..7, 14187 pixels static throughout."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_motion_cases as MC
import temporal_ref as T
from denoise_cases import bits, canaried, inner, rmse

pytestmark = pytest.mark.gpu

F32 = np.float32
# 1 x 1 has W - 1 = 0; 3 x 7 is narrower than a block; 33 x 17 is ragged on both axes; 70 x 130 spans several
# blocks on both axes (4 x 64 pixels each)
SHAPES = [(1, 1), (3, 7), (33, 17), (70, 130)]
P = T.DEFAULTS
NAMES = ("alpha", "alpha_m", "tau_n", "tau_z", "tau_a", "eps_a", "min_history", "w_min")


@pytest.fixture(scope="module")
def restated():
    """Inputs and the restatement's outputs for every shape and kind, computed once."""
    out = {}
    for W, H in SHAPES:
        for kind in MC.KINDS:
            C, F, cam, ids, motion, prev = MC.hostile(kind, W, H)
            out[(W, H, kind)] = (C, F, cam, ids, motion, prev,
                                 T.accumulate(C, F, cam, prev, ids=ids, motion=motion, diagnostics=True, **P))
    return out


def _gpu(C, F, cam, ids, motion, prev):
    """(state, out_color, out_var) of prt_temporal_accumulate_motion."""
    return TC.on_gpu(P, C, F, cam, prev, ids, motion)


def _same(got, want, what=""):
    for name, g, w in zip(("state", "colour", "variance"), got, want):
        g, w = bits(g).reshape(g.shape[0], g.shape[1], -1), bits(w).reshape(w.shape[0], w.shape[1], -1)
        diff = np.argwhere(np.any(g != w, axis=-1))
        assert len(diff) == 0, (what, name, len(diff), diff[:5], g[tuple(diff[0])], w[tuple(diff[0])])


@pytest.mark.parametrize("kind", MC.KINDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(restated, W, H, kind):
    C, F, cam, ids, motion, prev, (w_state, w_color, w_var, d) = restated[(W, H, kind)]
    assert list(P) == list(NAMES)
    _same(_gpu(C, F, cam, ids, motion, prev), (w_state, w_color, w_var))
    # the Python front end, with and without the colour
    from pyrenderer_amd import denoise as D
    s2, c2 = D.temporal_accumulate(C, F, cam, prev, ids=ids, motion=motion, **P)
    assert np.array_equal(bits(s2), bits(w_state)) and np.array_equal(bits(c2), bits(w_color))
    s3 = D.temporal_accumulate(C, F, cam, prev, ids=ids, motion=motion, return_color=False, **P)
    assert np.array_equal(bits(s3), bits(w_state))
    # what the inputs exercise
    if W * H > 500 and prev is not None:
        for v in MC.BAD_IDS:
            assert (ids == v).any() and (prev[3] == v).any()
        assert d["no_pose"].any() and not d["valid"][d["no_pose"]].any()
        if kind in ("static", "moved"):
            v = d["valid"]
            assert (v & (ids == MC.CARD)).any() and (v & (ids == MC.GROUND)).any() and (~v & (ids == MC.CARD)).any()
            assert (w_state[v, 3] > 1).all()
        if kind == "static":
            assert d["one_tap"].any() and (~d["one_tap"] & v).any() and (v & np.isin(ids, MC.BAD_IDS)).any()


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_without_ids_in_the_table_it_is_the_static_entry_point(W, H, kind):
    """All ids -1: prt_temporal_accumulate bit for bit on temporal_cases.hostile, with an empty table (NULL) and
    with one whose rows nobody may read."""
    from pyrenderer_amd import denoise as D
    C, F, cam, prev = TC.hostile(kind, W, H)
    want = D.temporal_accumulate(C, F, cam, prev, **P)
    none = np.full((W, H), -1, np.int32)
    mprev = None if prev is None else (*prev, none)
    for motion in (None, MC.motion_table()):
        state, color, _ = _gpu(C, F, cam, none, motion, mprev)
        assert np.array_equal(bits(state), bits(want[0])) and np.array_equal(bits(color), bits(want[1]))


def _int_plane(torch, dev, a, pad=64):
    """An int32 device plane between `pad` words of 7: (whole tensor, pointer to the plane, the host copy)."""
    host = np.concatenate([np.full(pad, 7, np.int32), a.reshape(-1), np.full(pad, 7, np.int32)])
    buf = torch.from_numpy(host).to(dev)
    return buf, buf.data_ptr() + pad * 4, host


def test_device_form_on_a_side_stream(restated):
    import torch
    from pyrenderer_amd import denoise as D
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    W, H = 70, 130
    n = W * H
    for kind in ("first", "moved", "static"):
        C, F, cam, ids, motion, prev, (w_state, w_color, w_var, _) = restated[(W, H, kind)]
        d_c, d_f = torch.from_numpy(C).to(dev), torch.from_numpy(F).to(dev)
        b_ids, p_ids, h_ids = _int_plane(torch, dev, ids)
        b_m, p_m = canaried(torch, dev, motion.size)
        b_m[64:64 + motion.size] = torch.from_numpy(motion.reshape(-1)).to(dev)
        h_m = b_m.cpu().numpy().copy()
        kw, b_pids = {}, None
        if prev is not None:
            d_ps, d_pf = torch.from_numpy(prev[0]).to(dev), torch.from_numpy(prev[1]).to(dev)
            b_pids, p_pids, h_pids = _int_plane(torch, dev, prev[3])
            kw = dict(d_prev_feat_ptr=d_pf.data_ptr(), prev_cam=prev[2], d_prev_state_ptr=d_ps.data_ptr(),
                      d_prev_ids_ptr=p_pids)
        b_state, p_state = canaried(torch, dev, n * 8)
        b_color, p_color = canaried(torch, dev, n * 3)
        b_var, p_var = canaried(torch, dev, n)
        stream.wait_stream(torch.cuda.current_stream(dev))
        D.temporal_accumulate_device(d_c.data_ptr(), d_f.data_ptr(), cam, W, H, p_state, d_out_color_ptr=p_color,
                                     d_out_var_ptr=p_var, stream_ptr=stream.cuda_stream, d_ids_ptr=p_ids,
                                     d_motion_ptr=p_m, n_objects=motion.shape[0], **P, **kw)
        stream.synchronize()
        assert np.array_equal(inner(b_state, n * 8).view(np.uint32), bits(w_state).reshape(-1)), kind
        assert np.array_equal(inner(b_color, n * 3).view(np.uint32), bits(w_color).reshape(-1)), kind
        assert np.array_equal(inner(b_var, n).view(np.uint32), bits(w_var).reshape(-1)), kind
        # the inputs, their canaries included, are as they were
        assert np.array_equal(bits(d_c.cpu().numpy()), bits(C)) and np.array_equal(bits(d_f.cpu().numpy()), bits(F))
        assert np.array_equal(b_ids.cpu().numpy(), h_ids) and np.array_equal(bits(b_m.cpu().numpy()), bits(h_m))
        if prev is not None:
            assert np.array_equal(b_pids.cpu().numpy(), h_pids)
            assert np.array_equal(bits(d_ps.cpu().numpy()), bits(prev[0]))
        # an empty table with a NULL pointer: every id is without a row, the id test stays
        want = T.accumulate(C, F, cam, prev, ids=ids, **P)
        b_state2, p_state2 = canaried(torch, dev, n * 8)
        D.temporal_accumulate_device(d_c.data_ptr(), d_f.data_ptr(), cam, W, H, p_state2, stream_ptr=stream.cuda_stream,
                                     d_ids_ptr=p_ids, d_motion_ptr=None, n_objects=0, **P, **kw)
        stream.synchronize()
        assert np.array_equal(inner(b_state2, n * 8).view(np.uint32), bits(want[0]).reshape(-1)), kind


# ------------------------------------------------------------ object ids ----

def test_object_ids_on_cornell(cornell, gpu_scene):
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.camera import PackedCamera
    scene, cam, flat = cornell
    W, H = 32, 24
    rec = cam.packed((W, H))
    ids = D.object_ids(gpu_scene, rec, W, H)
    assert ids.shape == (W, H) and ids.dtype == np.int32
    # the composition, restated: the pixel-centre rays of the kernel's formula through closest_hits and tri_prim
    u = (np.arange(W, dtype=F32) + F32(0.5)) / F32(W - 1)
    v = (np.arange(H, dtype=F32) + F32(0.5)) / F32(H - 1)
    o, d = PackedCamera.from_record(rec).gen_ray(u[:, None], v[None, :])
    hid, ht = gpu_scene.closest_hits(o.reshape(-1, 3), d.reshape(-1, 3), D.T_MIN, D.T_MAX)
    hid = hid.reshape(W, H)
    assert flat.sph.shape[0] == 0 and (hid < flat.n_tri).all()
    want = np.where(hid >= 0, flat.tri_prim[np.maximum(hid, 0)], -1)
    assert np.array_equal(ids, want)
    assert np.array_equal(ids == -1, hid < 0) and np.array_equal(ids == -1, ht.reshape(W, H) == 0)
    assert (ids == 5).any() and (ids == 6).any() and ids.max() < len(scene.primitives)
    # no pixel-centre ray exists: all -1, and nothing is traced (there is no scene to trace)
    for w, h in ((1, 9), (9, 1), (1, 1)):
        assert np.array_equal(D.object_ids(None, rec, w, h), np.full((w, h), -1, np.int32))


def test_object_ids_map_spheres_to_their_primitive():
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import build_world
    from denoise_cases import load_scene
    scene, cam = load_scene("specular")
    world = build_world(scene, (0,))
    flat = world.flat
    assert flat.sph.shape[0] >= 1 and (flat.sph_prim >= 0).all()
    for k, pid in enumerate(flat.sph_prim):
        assert getattr(scene.primitives[pid], "type_name", "") == "sphere"
        assert np.allclose(flat.sph[k, 0:3], scene.primitives[pid].center)
    ids = D.object_ids(world.device_scene(0), cam.packed((48, 48)), 48, 48)
    assert np.isin(flat.sph_prim, ids).all() and ids.max() < len(scene.primitives)


# -------------------------------------------------------------- end to end ----

BOX = 5               # the short box of the Cornell scene
FRAMES = 8
# measured on the MI355X (module docstring; DESIGN.md §11 "Moving objects")
SHARE = 0.9444        # the least measured share of the box's pixels that keep their history, frames 1..7
# RMSE(temporal accumulation with motion + variance filter) / RMSE(render(denoise="variance") of the last frame
# alone), both against a 1024-spp render of the last frame's scene; beside test_gpu_temporal.RHO = 0.2870.  The
# margin rule of test_gpu_denoise.test_it_denoises: sqrt(rho).
RHO_MOTION = 0.2481


def _scenes(scene):
    from pyrenderer_amd import scenes as S
    g = S.spin(scene.primitives[BOX], 6.0)
    g[:3, 3] += (0.0, 0.0, 0.02)
    out = [scene]
    for _ in range(1, FRAMES):
        out.append(S.moved(out[-1], {BOX: g}))
    return out


@pytest.fixture(scope="module")
def turning_box(cornell):
    """The 8-frame sequence: per frame the id plane, the history and the features; the last frame's images."""
    from pyrenderer_amd.core.tracing import TemporalAccumulator, build_world, render
    scene, cam, _ = cornell
    scenes = _scenes(scene)
    kw = dict(depth=8, seed=2, resolution=(128, 128))
    acc = TemporalAccumulator(scene, spp=1, **kw)
    frames = []
    for t in range(FRAMES):
        acc.add(cam, scenes[t])
        frames.append(dict(ids=acc.object_ids().copy(), h=acc.history().copy(), feat=acc.features().copy()))
    last_world = build_world(scenes[-1], (0,))
    return dict(frames=frames, temporal=acc.denoised(), accumulated=acc.accumulated().copy(), scenes=scenes, cam=cam,
                alone=render(scenes[-1], cam, spp=1, denoise="variance", world=last_world, **kw),
                ref=render(scenes[-1], cam, spp=1024, depth=8, seed=1, resolution=(128, 128), world=last_world))


def test_the_unchanged_scene_is_the_static_path(cornell):
    """A run that passes the unchanged scene to every add() equals the run that passes none, bit for bit."""
    from pyrenderer_amd.core.tracing import TemporalAccumulator, build_world
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    kw = dict(depth=4, seed=3, resolution=(64, 48), world=world, spp=1)
    plain, same = TemporalAccumulator(scene, **kw), TemporalAccumulator(scene, **kw)
    for t in range(4):
        plain.add(cam)
        same.add(cam, scene)
        assert np.array_equal(bits(plain.state()), bits(same.state())), t
        assert np.array_equal(bits(plain.accumulated()), bits(same.accumulated())), t
        assert np.array_equal(bits(plain.denoised()), bits(same.denoised())), t
    assert np.array_equal(plain.object_ids(), same.object_ids())
    assert (same.history()[same.features()[..., 7] > 0] == 4).all()


def test_what_follows_from_the_id_test(turning_box):
    """Static camera, so a static primitive's pixel takes its own previous state alone.  Where the box stood at
    that pixel in the previous frame, the history is exactly 1.  Where the id and the previous id agree on a static
    primitive and the one-sample features are the previous frame's bit for bit, the history is the previous one
    plus 1: t + 1 where that held in every frame.  (The id is the pixel-centre ray's, the features are the
    render's jittered sample 0 of the pixel: at the box's silhouette the two can see different primitives, so
    the features are asked for explicitly.  Such pixels lie on the box's silhouette in one of the two frames, at
    most twice its perimeter of some 200 pixels among more than 12 000 static ones: at least 0.9 must agree.)"""
    fr = turning_box["frames"]
    uncovered_total, always = 0, np.ones((128, 128), bool)
    assert (fr[0]["h"] == 1).all()
    for t in range(1, FRAMES):
        ids, pids, h, ph = fr[t]["ids"], fr[t - 1]["ids"], fr[t]["h"], fr[t - 1]["h"]
        uncovered = (ids != BOX) & (pids == BOX)
        uncovered_total += int(uncovered.sum())
        assert (h[uncovered] == 1).all(), t
        agree = (ids == pids) & (ids != BOX) & (ids >= 0)
        stable = agree & (bits(fr[t]["feat"]) == bits(fr[t - 1]["feat"])).all(-1) & (fr[t]["feat"][..., 7] > 0)
        assert stable.sum() >= 0.9 * agree.sum(), (t, stable.sum(), agree.sum())
        assert np.array_equal(h[stable], ph[stable] + 1), t
        always &= stable
        assert always.sum() > 0.5 * 128 * 128 and (h[always] == t + 1).all(), t
    print(f"turning box: {uncovered_total} uncovered pixels in frames 1..7, {int(always.sum())} pixels static throughout")
    assert uncovered_total >= 20


def test_the_box_keeps_its_history_and_the_sequence_beats_the_last_frame_alone(turning_box):
    t = turning_box
    shares = []
    for f in t["frames"]:
        box = (f["ids"] == BOX) & (f["feat"][..., 7] > 0)
        assert box.sum() > 300
        shares.append(float((f["h"][box] > 1).mean()))
    print("turning box history shares of the box's pixels, frames 0..7:", " ".join(f"{s:.4f}" for s in shares))
    e_t, e_a = rmse(t["temporal"], t["ref"]), rmse(t["alone"], t["ref"])
    print(f"turning box quality cornell 128^2 1 spp 8 frames: rmse temporal {e_t:.6f} alone {e_a:.6f} ratio {e_t / e_a:.4f}")
    assert shares[0] == 0.0 and min(shares[1:]) >= SHARE - 0.05, shares
    assert np.isfinite(t["temporal"]).all() and np.isfinite(t["accumulated"]).all()
    assert e_t < e_a, (e_t, e_a)
    assert e_t / e_a <= np.sqrt(RHO_MOTION), (e_t / e_a, RHO_MOTION)


def test_render_sequence_and_the_command_line_are_the_stepwise_accumulator(cornell, tmp_path):
    """render_sequence(..., scenes=...) and --frames 3 --spin 5 6 --temporal are TemporalAccumulator.add(camera,
    scene) frame by frame, over pyrenderer_amd.scenes.spun's scenes."""
    import os
    from pyrenderer_amd import scenes as S
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    from pyrenderer_amd.main import main
    scene, cam, _ = cornell
    scenes = S.spun(scene, BOX, 6.0, 3)
    kw = dict(spp=2, depth=4, seed=5, resolution=(32, 24))
    step = TemporalAccumulator(scene, **kw)
    raw, seq = [], []
    for s in scenes:
        step.add(cam, s)
        raw.append(step.accumulated().copy())
        seq.append(step.denoised())
    assert (step.object_ids() == BOX).any() and (step.history()[step.object_ids() == BOX] > 1).any()
    got = render_sequence(scene, [cam] * 3, scenes=scenes, **kw)
    assert np.array_equal(bits(got), bits(np.stack(seq)))
    got = render_sequence(scene, [cam] * 3, scenes=scenes, denoise=False, **kw)
    assert np.array_equal(bits(got), bits(np.stack(raw)))
    argv = ["--resolution", "32", "24", "--depth", "4", "--seed", "5", "--samples", "2", "--frames", "3", "--spin",
            str(BOX), "6", "--temporal"]
    last = main(argv + ["--out", str(tmp_path / "s.png"), "--denoise", "--denoise-mode", "variance"])
    assert sorted(os.listdir(tmp_path)) == ["s.0000.png", "s.0001.png", "s.0002.png"]
    assert np.array_equal(bits(last), bits(seq[-1]))
    assert np.array_equal(bits(main(argv + ["--out", ""])), bits(raw[-1]))
    # the box really moved: the static sequence differs
    still = render_sequence(scene, [cam] * 3, denoise=False, **kw)
    assert not np.array_equal(still[-1], raw[-1])

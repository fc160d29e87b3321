"""Temporal accumulation on the GPU: prt_temporal_accumulate and prt_denoise_var_mixed against the NumPy
restatement (tests/temporal_ref.py) bit for bit, the device entry points, and a Cornell turntable end to end.

Measured on the MI355X for the end-to-end sequence below (Cornell 128^2, 1 spp, depth 8, 8 frames at 2 degrees
per frame, default parameters): RMSE 0.015461 with the history against 0.053877 for the last frame alone,
ratio 0.2870 (RHO); hit pixels with history in frames 1..7: 0.9649 to 0.9875."""
import numpy as np
import pytest

import atrous_ref as R
import atrous_var_ref as V
import moments_ref as M
import temporal_cases as TC
import temporal_ref as T
from denoise_cases import MARKER, bits, canaried, inner, mixed_inputs, rmse

pytestmark = pytest.mark.gpu

F32 = np.float32
# 1 x 1 has W - 1 = 0; 3 x 7 is narrower than a block; 33 x 17 is ragged on both axes; 70 x 130 spans several
# blocks on both axes (4 x 64 pixels each)
SHAPES = [(1, 1), (3, 7), (33, 17), (70, 130)]
P = T.DEFAULTS
PAR = dict(sigma_l=1.5, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3, eps_l=3e-3)


@pytest.fixture(scope="module")
def restated():
    """Inputs and the restatement's outputs for every shape and kind, computed once."""
    out = {}
    for W, H in SHAPES:
        for kind in TC.KINDS:
            C, F, cam, prev = TC.hostile(kind, W, H)
            out[(W, H, kind)] = (C, F, cam, prev, T.accumulate(C, F, cam, prev, diagnostics=True, **P))
    return out


def _gpu(C, F, cam, prev, **kw):
    """(state, out_color, out_var) of prt_temporal_accumulate with P, but for the parameters in `kw`."""
    return TC.on_gpu({**P, **kw}, C, F, cam, prev)


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_kernel_equals_the_restatement_bit_for_bit(restated, W, H, kind):
    C, F, cam, prev, (w_state, w_color, w_var, d) = restated[(W, H, kind)]
    assert list(P) == ["alpha", "alpha_m", "tau_n", "tau_z", "tau_a", "eps_a", "min_history", "w_min"]
    state, color, var = _gpu(C, F, cam, prev)
    for name, got, want in (("state", state, w_state), ("colour", color, w_color), ("variance", var[..., None], w_var[..., None])):
        diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
        assert len(diff) == 0, (name, len(diff), diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])
    # the Python front end, with and without the colour
    from pyrenderer_amd import denoise as D
    s2, c2 = D.temporal_accumulate(C, F, cam, prev, **P)
    assert np.array_equal(bits(s2), bits(w_state)) and np.array_equal(bits(c2), bits(w_color))
    assert np.array_equal(bits(D.temporal_accumulate(C, F, cam, prev, return_color=False, **P)), bits(w_state))
    # what the inputs exercise
    if W * H > 500:
        bad = T.prepare(C, F, P["eps_a"])[6]   # a colour of 3e38 over an albedo below 1 overflows: bad as well
        hit = F[..., 7] > 0
        assert bad.any() and (bad & np.isfinite(C).all(-1) & np.isfinite(F).all(-1)).any() and (~hit).any() and (F[..., 0] < P["eps_a"]).any() and (np.abs(F[..., 6]) == F32(1e30)).any()
        assert not state[bad].any() and (bits(var[bad]) == MARKER).all()
        assert (state[~hit & ~bad, 3] == 1).all()
        if kind == "first":
            assert (state[~bad, 3] == 1).all() and (bits(var) == MARKER).all()
        if kind in ("static", "moved"):
            ps, pf, _ = prev
            assert (ps[..., 3] == 0).any() and (pf[..., 7] == 0).any()
            v = d["valid"]
            assert 0.3 < v.mean() < 0.8 and (state[v, 3] > 1).all() and (state[~v & ~bad, 3] == 1).all()
            known = bits(var) != MARKER
            assert known.any() and (known <= v).all() and (var[known] >= 0).all()
            assert (state[v, 3] >= P["min_history"])[known[v]].all()
        if kind == "moved":
            px, py, r = d["px"], d["py"], d["in_range"]
            for lo, hi, q in ((-1, 0, px), (W - 1, W, px), (-1, 0, py), (H - 1, H, py)):
                assert ((q > lo) & (q < hi) & r).any(), (lo, hi)   # taps on both sides of every border
        if kind == "behind":
            assert d["valid"].mean() < 0.05
            plain = hit & ~bad & (F[..., 6] > 0)
            assert not d["in_range"][plain].any() and (state[plain, 3] == 1).all()


@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1)])
def test_one_row_and_one_column_frames(W, H):
    """W - 1 = 0 or H - 1 = 0 divides by zero in the pixel-centre ray: a moved camera resets every pixel, a
    static one still accumulates, and nothing faults."""
    rng = np.random.default_rng(W + 2 * H)
    cam, pcam = TC.cameras("moved", W, H)
    F = TC.plane_features(cam, W, H)
    C = rng.random((W, H, 3), dtype=F32)
    S = TC.random_state(rng, W, H)
    assert F[..., 7].all()
    for prev_cam, h_want in ((pcam, np.ones((W, H), F32)), (cam.copy(), S[..., 3] + 1)):
        want = T.accumulate(C, F, cam, (S, F, prev_cam), **P)
        got = _gpu(C, F, cam, (S, F, prev_cam))
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w))
        assert np.array_equal(got[0][..., 3], h_want)


def test_a_static_sequence_is_a_running_mean_on_the_gpu():
    W, H, n = 33, 17, 6
    rng = np.random.default_rng(5)
    _, cam = TC.camera((0.3, 0.2, 4.0), resolution=(W, H))
    F = TC.plane_features(cam, W, H)
    frames = [rng.random((W, H, 3), dtype=F32) * F32(2.0) for _ in range(n)]
    prev = None
    for C in frames:
        state, _, _ = _gpu(C, F, cam, prev, alpha=0.0, alpha_m=0.0)
        prev = (state, F, cam)
    I = np.stack([C.astype(np.float64) / F[..., 0:3] for C in frames])
    assert (state[..., 3] == n).all()
    assert np.abs(state[..., 0:3] - I.mean(0)).max() <= n * 4 * 2.0 ** -24 * np.abs(I).max()


def test_device_form_equals_the_host_form(restated):
    import torch
    from pyrenderer_amd import denoise as D
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    W, H = 70, 130
    n = W * H
    for kind in ("first", "moved", "static"):
        C, F, cam, prev, (w_state, w_color, w_var, _) = restated[(W, H, kind)]
        d_c, d_f = torch.from_numpy(C).to(dev), torch.from_numpy(F).to(dev)
        kw = {}
        if prev is not None:
            d_ps, d_pf = torch.from_numpy(prev[0]).to(dev), torch.from_numpy(prev[1]).to(dev)
            kw = dict(d_prev_feat_ptr=d_pf.data_ptr(), prev_cam=prev[2], d_prev_state_ptr=d_ps.data_ptr())
        b_state, p_state = canaried(torch, dev, n * 8)
        b_color, p_color = canaried(torch, dev, n * 3)
        b_var, p_var = canaried(torch, dev, n)
        stream.wait_stream(torch.cuda.current_stream(dev))
        D.temporal_accumulate_device(d_c.data_ptr(), d_f.data_ptr(), cam, W, H, p_state, d_out_color_ptr=p_color,
                                     d_out_var_ptr=p_var, stream_ptr=stream.cuda_stream, **P, **kw)
        stream.synchronize()
        assert np.array_equal(inner(b_state, n * 8).view(np.uint32), bits(w_state).reshape(-1)), kind
        assert np.array_equal(inner(b_color, n * 3).view(np.uint32), bits(w_color).reshape(-1)), kind
        assert np.array_equal(inner(b_var, n).view(np.uint32), bits(w_var).reshape(-1)), kind
        assert np.array_equal(bits(d_c.cpu().numpy()), bits(C)) and np.array_equal(bits(d_f.cpu().numpy()), bits(F))
        # the optional outputs left out: the state alone, the other buffers untouched
        b_state2, p_state2 = canaried(torch, dev, n * 8)
        D.temporal_accumulate_device(d_c.data_ptr(), d_f.data_ptr(), cam, W, H, p_state2, stream_ptr=stream.cuda_stream,
                                     **P, **kw)
        stream.synchronize()
        assert np.array_equal(inner(b_state2, n * 8).view(np.uint32), bits(w_state).reshape(-1)), kind


# ------------------------------------------------------ prt_denoise_var_mixed ----

@pytest.mark.parametrize("W,H", SHAPES)
def test_mixed_variance_equals_the_restatement_and_its_two_limits(W, H):
    from pyrenderer_amd.denoise import denoise_variance
    C, F, plane = mixed_inputs(W, H, 40 + W)
    for n in (0, 5):
        want, want_used = T.atrous_var_mixed(C, F, plane, n, **PAR)
        got, used = denoise_variance(C, F, iterations=n, variance=plane, variance_fallback="spatial",
                                     return_variance=True, **PAR)
        diff = np.argwhere(bits(used) != bits(want_used))
        assert len(diff) == 0, ("variance", n, len(diff), diff[:5])
        diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
        assert len(diff) == 0, ("image", n, len(diff), diff[:5])
        assert np.array_equal(bits(got), bits(denoise_variance(C, F, iterations=n, variance=plane,
                                                                 variance_fallback="spatial", **PAR)))   # no out_var
        assert np.isfinite(used).all() and (used >= 0).all()
    # all NaN: the spatial mode; all finite and >= 0: the given variance — both bit for bit, variance included
    nan = np.full((W, H), np.nan, F32)
    a = denoise_variance(C, F, variance=nan, variance_fallback="spatial", return_variance=True, **PAR)
    b = denoise_variance(C, F, return_variance=True, **PAR)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    full = np.where(np.isfinite(plane) & (plane >= 0), plane, F32(0.01)).astype(F32)
    a = denoise_variance(C, F, variance=full, variance_fallback="spatial", return_variance=True, **PAR)
    b = denoise_variance(C, F, variance=full, return_variance=True, **PAR)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    # "zero" stays today's path: the marker counts as 0
    z = denoise_variance(C, F, variance=plane, return_variance=True, **PAR)
    ref = M.atrous_var_given(C, F, plane, 5, **PAR)
    assert np.array_equal(bits(z[0]), bits(ref[0])) and np.array_equal(bits(z[1]), bits(ref[1]))
    if W * H > 500:
        live = (F[..., 7] > 0) & np.isfinite(C).all(-1) & np.isfinite(F).all(-1)
        gaps = live & ~(np.isfinite(plane) & (plane >= 0))
        assert gaps.sum() > 100 and (a[1][gaps] != z[1][gaps]).any()


def test_mixed_device_form_on_a_side_stream():
    import torch
    from pyrenderer_amd import denoise as D
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    W, H = 70, 130
    C, F, plane = mixed_inputs(W, H, 40 + W)
    want, want_used = T.atrous_var_mixed(C, F, plane, 5, **PAR)
    d_c, d_f, d_iv = (torch.from_numpy(a).to(dev) for a in (C, F, plane))
    b_out, p_out = canaried(torch, dev, W * H * 3)
    b_var, p_var = canaried(torch, dev, W * H)
    need = D.work_bytes_variance(W, H)
    d_work = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)   # exactly the spatial mode's scratch
    stream.wait_stream(torch.cuda.current_stream(dev))
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, p_out, d_work.data_ptr(), need, d_out_var_ptr=p_var,
                              d_in_var_ptr=d_iv.data_ptr(), variance_fallback="spatial", iterations=5,
                              stream_ptr=stream.cuda_stream, **PAR)
    stream.synchronize()
    assert np.array_equal(inner(b_out, W * H * 3).view(np.uint32), bits(want).reshape(-1))
    assert np.array_equal(inner(b_var, W * H).view(np.uint32), bits(want_used).reshape(-1))
    assert np.array_equal(bits(d_iv.cpu().numpy()), bits(plane))   # the input plane is left alone


# -------------------------------------------------------------- end to end ----

# RMSE(temporal accumulation + variance filter) / RMSE(render(denoise="variance") of the last frame alone), both
# against a 1024-spp render of the last camera: Cornell 128^2, 1 spp, depth 8, 8 frames at 2 degrees per frame,
# default parameters, measured on the MI355X.  The margin rule of
# test_gpu_denoise.test_it_denoises: sqrt(rho).
RHO = 0.2870


@pytest.fixture(scope="module")
def turntable(cornell):
    """The 8-frame sequence, then one jump of 40 degrees: per frame the share of hit pixels with history, the
    last regular frame's images, and the accumulator standing after the jump."""
    from pyrenderer_amd.core.camera import orbit
    from pyrenderer_amd.core.tracing import TemporalAccumulator, build_world, render
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    kw = dict(depth=8, seed=2, resolution=(128, 128), world=world)
    acc = TemporalAccumulator(scene, spp=1, **kw)
    shares = []
    for t in range(8):
        acc.add(orbit(cam, 2.0 * t))
        hit = acc.features()[..., 7] > 0
        shares.append(float((acc.history()[hit] > 1).mean()))
    last = orbit(cam, 14.0)
    out = dict(shares=shares, temporal=acc.denoised(), accumulated=acc.accumulated().copy(),
               alone=render(scene, last, spp=1, denoise="variance", **kw),
               ref=render(scene, last, spp=1024, depth=8, seed=1, resolution=(128, 128), world=world))
    acc.add(orbit(cam, 54.0))
    out.update(acc=acc, scene=scene, cam=cam, world=world)
    return out


def test_turntable_keeps_its_history_and_beats_the_last_frame_alone(turntable):
    t = turntable
    print("temporal history shares, frames 0..7:", " ".join(f"{s:.4f}" for s in t["shares"]))
    e_t, e_a = rmse(t["temporal"], t["ref"]), rmse(t["alone"], t["ref"])
    print(f"temporal quality cornell 128^2 1 spp 8 frames: rmse temporal {e_t:.6f} alone {e_a:.6f} ratio {e_t / e_a:.4f}")
    assert t["shares"][0] == 0.0 and min(t["shares"][1:]) >= 0.9, t["shares"]
    assert np.isfinite(t["temporal"]).all() and np.isfinite(t["accumulated"]).all()
    assert e_t < e_a, (e_t, e_a)
    assert e_t / e_a <= np.sqrt(RHO), (e_t / e_a, RHO)


def test_a_jump_resets_to_this_frames_colour(turntable):
    from pyrenderer_amd import denoise as D
    acc = turntable["acc"]
    state, feat, mean = acc.state(), acc.features(), acc.mean()
    I, _, _, _, _, hit, bad, a = R.prepass(mean, feat, D.EPS_A)
    h = acc.history()
    assert not bad.any() and np.isfinite(state[..., 0:6]).all()
    fresh = hit & (h == 1)
    print(f"temporal jump of 40 degrees: fresh {fresh.sum()} of {hit.sum()} hit pixels")
    assert fresh.sum() > 0.05 * hit.sum() and (hit & (h > 1)).sum() > 0.05 * hit.sum()
    assert np.array_equal(bits(state[fresh, 0:3]), bits(I[fresh]))
    assert (bits(state[fresh, 6]) == MARKER).all()
    assert np.isfinite(acc.accumulated()).all() and np.isfinite(acc.denoised()).all()
    # render_sequence is the same route: the jump's frame again, from a fresh history
    assert (h[~hit] == 1).all()


def test_render_sequence_and_a_static_accumulator(turntable):
    from pyrenderer_amd.core.camera import orbit
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    scene, cam, world = turntable["scene"], turntable["cam"], turntable["world"]
    kw = dict(depth=4, seed=3, resolution=(64, 48), world=world)
    acc = TemporalAccumulator(scene, spp=2, alpha=0.0, alpha_m=0.0, **kw)
    for _ in range(4):
        acc.add(cam)
    hit = acc.features()[..., 7] > 0
    assert hit.any() and (acc.history()[hit] == 4).all() and (acc.history()[~hit] == 1).all()
    # with alpha 0 the accumulated colour of a static camera is the mean of the four frames
    frames = []
    plain = TemporalAccumulator(scene, spp=2, **kw)
    for _ in range(4):
        frames.append(plain.add(cam).reset().mean())
    assert (plain.history() == 1).all()                      # reset() drops the history every time
    mean4 = np.mean(np.stack(frames).astype(np.float64), axis=0)
    assert np.allclose(acc.accumulated()[hit], mean4[hit], rtol=1e-4, atol=1e-6)
    cams = [orbit(cam, 3.0 * t) for t in range(3)]
    seq = render_sequence(scene, cams, spp=2, **kw)
    raw = render_sequence(scene, cams, spp=2, denoise=False, **kw)
    assert seq.shape == raw.shape == (3, 64, 48, 3) and seq.dtype == np.float32
    assert np.isfinite(seq).all() and np.isfinite(raw).all() and not np.array_equal(seq[2], raw[2])
    step = TemporalAccumulator(scene, spp=2, **kw)
    for t, c in enumerate(cams):
        step.add(c)
        assert np.array_equal(bits(step.accumulated()), bits(raw[t])) and np.array_equal(bits(step.denoised()), bits(seq[t]))


def test_command_line_writes_a_turntable(turntable, tmp_path):
    """--frames N --orbit DEG --temporal is render_sequence over core.camera.orbit's cameras; without --temporal
    every frame stands alone."""
    import os
    from pyrenderer_amd.core.camera import orbit
    from pyrenderer_amd.core.tracing import render_sequence
    from pyrenderer_amd.main import main
    scene, cam, world = turntable["scene"], turntable["cam"], turntable["world"]
    argv = ["--resolution", "32", "24", "--depth", "4", "--seed", "5", "--samples", "2", "--frames", "3", "--orbit", "3"]
    var = ["--denoise", "--denoise-mode", "variance"]
    cams = [orbit(cam, 3.0 * t) for t in range(3)]
    kw = dict(spp=2, depth=4, seed=5, resolution=(32, 24), world=world)
    last = main(argv + ["--temporal", "--out", str(tmp_path / "t.png")] + var)
    assert sorted(os.listdir(tmp_path)) == ["t.0000.png", "t.0001.png", "t.0002.png"]
    assert np.array_equal(bits(last), bits(render_sequence(scene, cams, **kw)[-1]))
    raw = main(argv + ["--temporal", "--out", ""])
    assert np.array_equal(bits(raw), bits(render_sequence(scene, cams, denoise=False, **kw)[-1]))
    alone = main(argv + ["--out", ""] + var)       # no history: the third frame's own two samples, filtered
    assert np.isfinite(alone).all() and not np.array_equal(alone, last)
    assert sorted(os.listdir(tmp_path)) == ["t.0000.png", "t.0001.png", "t.0002.png"]

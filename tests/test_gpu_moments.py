"""Variance from per-pixel sample moments on the GPU: prt_moments_add and prt_denoise_var_given against
the NumPy restatement (tests/moments_ref.py) bit for bit, the device entry points, the public API end to
end and the quality gain."""
import os

import numpy as np
import pytest

import atrous_ref as R
import atrous_var_ref as V
import moments_ref as M
import temporal_ref as T
from conftest import CORNELL_JSON
from denoise_cases import bits, mixed_inputs, reference, rmse
from moments_cases import BOUND, N_SAMPLES, PAR, features, frames

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
# 3 x 7 is narrower than the 5 x 5 stencil; 70 x 130 spans several blocks on both axes (4 x 64 pixels each)
SHAPES = [(1, 1), (3, 7), (33, 17), (70, 130)]


@pytest.fixture(scope="module")
def restated_moments():
    """Frames, features and the restatement's state for every shape and frame count, computed once."""
    out = {}
    for W, H in SHAPES:
        for K in (1, 2, 5):
            S, F = frames(W, H, K, 300 + 10 * W + K)
            out[(W, H, K)] = (S, F, M.moments_add(np.zeros((W, H, 4), F32), S, N_SAMPLES, F, PAR["eps_a"]))
    return out


def _padded(S, pad):
    """The frames with `pad` floats of 7.0 after each: (buffer, frame_pitch)."""
    K = S.shape[0]
    pitch = S[0].size + pad
    buf = np.full(K * pitch, 7.0, F32)
    for f in range(K):
        buf[f * pitch: f * pitch + S[0].size] = S[f].reshape(-1)
    return buf, pitch


@pytest.mark.parametrize("W,H", SHAPES)
def test_moments_equal_the_restatement_bit_for_bit(restated_moments, W, H):
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.denoise import moments_add, moments_state
    for K in (1, 2, 5):
        S, F, want = restated_moments[(W, H, K)]
        got = moments_add(moments_state(W, H), S, N_SAMPLES, F, eps_a=PAR["eps_a"])
        diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
        assert len(diff) == 0, (K, len(diff), diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])
        # a non-zero frame pitch
        buf, pitch = _padded(S, 5)
        st = moments_state(W, H)
        N.check_denoise(N.lib().prt_moments_add(0, N.ptr(buf), K, pitch, N_SAMPLES, N.ptr(F), PAR["eps_a"], W, H, N.ptr(st)))
        assert np.array_equal(bits(st), bits(want)), K
        # split over two calls
        if K > 1:
            st = moments_state(W, H)
            moments_add(st, S[:K // 2], N_SAMPLES, F, eps_a=PAR["eps_a"])
            assert (st[..., 0] <= K // 2).all()
            moments_add(st, S[K // 2:], N_SAMPLES, F, eps_a=PAR["eps_a"])
            assert np.array_equal(bits(st), bits(want)), K
        # what the inputs exercise: the bound stays finite, the non-finite frames are skipped
        assert np.isfinite(got).all() and (got[..., 3] >= 0).all()
        assert got[W - 1, H - 1, 0] == K and (K < 2 or got[W - 1, H - 1, 2] >= BOUND * BOUND)
        if W * H >= 4:
            assert (got[..., 0] == K).sum() == W * H - 2 and (got[..., 0] == K - 1).sum() == 2
            assert (F[..., 7] == 0).any() and (F[..., 0] < PAR["eps_a"]).any()
        if K == 1:
            assert not got[..., 2:4].any()
        elif W * H > 100:
            assert np.mean(got[..., 3] > 0) > 0.95


def _given_inputs(W, H, seed):
    """Colour, features and a variance plane with a NaN, an inf and a -1 at hit pixels (from 4 pixels on)."""
    rng = np.random.default_rng(seed)
    F = features(W, H, rng)
    amp = np.where(np.arange(W)[:, None, None] < (W + 1) // 2, 0.05, 0.6)
    C = (F[..., 0:3] * (1.0 + amp * rng.uniform(-1.0, 1.0, (W, H, 3)))).astype(F32)
    iv = (rng.uniform(0.0, 0.3, (W, H)) ** 2).astype(F32)
    clean = iv.copy()
    if W * H >= 4:
        hits = np.argwhere(F[..., 7] > 0)
        C[tuple(hits[len(hits) // 7])] = (np.nan, 0.1, 0.2)   # a set-aside pixel
        for j, v in enumerate((np.nan, np.inf, -1.0)):
            x, y = hits[(j + 1) * len(hits) // 5]
            iv[x, y] = v
            clean[x, y] = 0.0
    return C, F, iv, clean


@pytest.fixture(scope="module")
def restated_given():
    out = {}
    for W, H in SHAPES:
        C, F, iv, clean = _given_inputs(W, H, 500 + W)
        out[(W, H)] = (C, F, iv, clean, {n: M.atrous_var_given(C, F, iv, n, **PAR) for n in (0, 1, 5, 8)})
    return out


@pytest.mark.parametrize("W,H", SHAPES)
def test_given_variance_filter_equals_the_restatement_bit_for_bit(restated_given, W, H):
    from pyrenderer_amd.denoise import denoise_variance
    C, F, iv, clean, want = restated_given[(W, H)]
    live = (F[..., 7] > 0) & np.isfinite(C).all(axis=-1)
    for n in (0, 1, 5, 8):
        got, used = denoise_variance(C, F, iterations=n, return_variance=True, variance=iv, **PAR)
        diff = np.argwhere(bits(used) != bits(want[n][1]))
        assert len(diff) == 0, ("variance", n, len(diff), diff[:5])
        diff = np.argwhere(np.any(bits(got) != bits(want[n][0]), axis=-1))
        assert len(diff) == 0, ("image", n, len(diff), diff[:5])
        assert np.array_equal(bits(got), bits(denoise_variance(C, F, iterations=n, variance=iv, **PAR)))   # no out_var
        assert np.isfinite(used).all() and (used >= 0).all() and not used[~live].any()
        assert np.array_equal(bits(used[live]), bits(clean[live]))
    # NaN, inf and -1 behave as 0
    a = denoise_variance(C, F, iterations=5, variance=iv, **PAR)
    b = denoise_variance(C, F, iterations=5, variance=clean, **PAR)
    assert np.array_equal(bits(a), bits(b))
    if W * H > 100:   # and the plane is at work: another variance, another image
        c = denoise_variance(C, F, iterations=5, variance=clean * F32(16.0), **PAR)
        assert np.mean(np.any(a[live] != c[live], axis=-1)) > 0.5


@pytest.mark.parametrize("W,H", [(33, 17), (70, 130)])
def test_the_spatial_estimate_fed_back_reproduces_the_spatial_mode(restated_given, W, H):
    from pyrenderer_amd.denoise import denoise_variance
    C, F, _, _, _ = restated_given[(W, H)]
    img, est = denoise_variance(C, F, iterations=5, return_variance=True, **PAR)
    again, used = denoise_variance(C, F, iterations=5, return_variance=True, variance=est, **PAR)
    assert np.array_equal(bits(img), bits(again)) and np.array_equal(bits(est), bits(used))
    want, want_est = V.atrous_var(C, F, 5, **PAR)
    assert np.array_equal(bits(img), bits(want)) and np.array_equal(bits(est), bits(want_est))
    mz = est.copy()
    mz[0, 0] = -0.0   # the restatement passes a -0 on as -0 at a usable pixel, as +0 elsewhere
    got = denoise_variance(C, F, iterations=2, return_variance=True, variance=mz, **PAR)
    ref = M.atrous_var_given(C, F, mz, 2, **PAR)
    assert np.array_equal(bits(got[0]), bits(ref[0])) and np.array_equal(bits(got[1]), bits(ref[1]))


def test_device_entry_points_on_a_side_stream(restated_moments, restated_given):
    import torch
    from pyrenderer_amd import denoise as D
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    W, H, K = 70, 130, 5
    S, F, want = restated_moments[(W, H, K)]
    buf, pitch = _padded(S, 12)
    d_s, d_f = torch.from_numpy(buf).to(dev), torch.from_numpy(F).to(dev)
    d_state = torch.zeros((W, H, 4), dtype=torch.float32, device=dev)
    assert d_state.data_ptr() % 16 == 0
    stream.wait_stream(torch.cuda.current_stream(dev))
    # two enqueues on the stream: frames 0..1, then 2..4 from an offset base pointer
    D.moments_add_device(d_s.data_ptr(), 2, N_SAMPLES, d_f.data_ptr(), W, H, d_state.data_ptr(), frame_pitch=pitch,
                         eps_a=PAR["eps_a"], stream_ptr=stream.cuda_stream)
    D.moments_add_device(d_s.data_ptr() + 2 * pitch * 4, 3, N_SAMPLES, d_f.data_ptr(), W, H, d_state.data_ptr(),
                         frame_pitch=pitch, eps_a=PAR["eps_a"], stream_ptr=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(bits(d_state.cpu().numpy()), bits(want))
    assert (d_s.cpu().numpy().reshape(K, pitch)[:, -12:] == 7.0).all()

    C, F, iv, _, wants = restated_given[(W, H)]
    want_img, want_used = wants[5]
    d_c, d_f, d_iv = (torch.from_numpy(a).to(dev) for a in (C, F, iv))
    d_out = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    d_var = torch.full((W, H), -1.0, dtype=torch.float32, device=dev)
    need = D.work_bytes_variance(W, H)
    d_work = torch.empty(need, dtype=torch.uint8, device=dev)   # exactly the spatial mode's scratch
    stream.wait_stream(torch.cuda.current_stream(dev))
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(), need,
                              d_out_var_ptr=d_var.data_ptr(), d_in_var_ptr=d_iv.data_ptr(), iterations=5,
                              stream_ptr=stream.cuda_stream, **PAR)
    stream.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(want_img))
    assert np.array_equal(bits(d_var.cpu().numpy()), bits(want_used))
    assert np.array_equal(bits(d_iv.cpu().numpy()), bits(iv))   # the input plane is left alone
    d_var.fill_(-1.0)
    torch.cuda.synchronize(dev)
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(), need,
                              d_in_var_ptr=d_iv.data_ptr(), iterations=5, stream_ptr=stream.cuda_stream, **PAR)
    stream.synchronize()
    assert np.array_equal(bits(d_out.cpu().numpy()), bits(want_img)) and (d_var.cpu().numpy() == -1.0).all()


def test_modes_alternating_on_one_scratch_leave_nothing_behind(restated_given):
    """The modes share their launch and scratch code: given variance, fixed, mixed (a plane with NaN gaps, whose
    estimate kernel writes the planes the others read), spatial estimate and fixed again on one NaN-filled
    scratch and one stream, with no host synchronisation in between.  A plane that one mode left behind and
    the next one read would show in the bits."""
    import torch
    from pyrenderer_amd import denoise as D
    fixed_par = dict(sigma_c=1.5, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3)   # test_gpu_denoise.py's
    W, H = 70, 130
    C, F, iv, _, wants = restated_given[(W, H)]
    want_given = wants[5][0]
    want_fixed = R.atrous(C, F, 5, **fixed_par)
    want_spatial = V.atrous_var(C, F, 5, **PAR)[0]
    plane = mixed_inputs(W, H, 40 + W)[2]   # test_gpu_temporal.py's: the marker on about half of the pixels
    want_mixed = T.atrous_var_mixed(C, F, plane, 5, **PAR)[0]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    d_c, d_f, d_iv, d_plane = (torch.from_numpy(a).to(dev) for a in (C, F, iv, plane))
    need_var, need_fixed = D.work_bytes_variance(W, H), D.work_bytes(W, H)
    assert need_fixed < need_var
    d_work = torch.full((need_var,), 0xFF, dtype=torch.uint8, device=dev)
    assert d_work.data_ptr() % 16 == 0
    outs = [torch.zeros((W, H, 3), dtype=torch.float32, device=dev) for _ in range(5)]
    stream.wait_stream(torch.cuda.current_stream(dev))
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, outs[0].data_ptr(), d_work.data_ptr(), need_var,
                              d_in_var_ptr=d_iv.data_ptr(), iterations=5, stream_ptr=stream.cuda_stream, **PAR)
    D.denoise_device(d_c.data_ptr(), d_f.data_ptr(), W, H, outs[1].data_ptr(), d_work.data_ptr(), need_fixed,
                     iterations=5, stream_ptr=stream.cuda_stream, **fixed_par)
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, outs[2].data_ptr(), d_work.data_ptr(), need_var,
                              d_in_var_ptr=d_plane.data_ptr(), variance_fallback="spatial", iterations=5,
                              stream_ptr=stream.cuda_stream, **PAR)
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, outs[3].data_ptr(), d_work.data_ptr(), need_var,
                              iterations=5, stream_ptr=stream.cuda_stream, **PAR)
    D.denoise_device(d_c.data_ptr(), d_f.data_ptr(), W, H, outs[4].data_ptr(), d_work.data_ptr(), need_fixed,
                     iterations=5, stream_ptr=stream.cuda_stream, **fixed_par)
    stream.synchronize()
    for name, got, want in zip(("given", "fixed", "mixed", "spatial", "fixed again"), outs,
                               (want_given, want_fixed, want_mixed, want_spatial, want_fixed)):
        diff = np.argwhere(np.any(bits(got.cpu().numpy()) != bits(want), axis=-1))
        assert len(diff) == 0, (name, len(diff), diff[:5])


# -------------------------------------------------------------- end to end ----

def test_render_and_accumulator_agree_end_to_end(cornell, tmp_path):
    """Cornell 64^2, K = 4 batches of 2 spp."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import Accumulator, build_world, render, render_batches
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    K, n = 4, 2
    kw = dict(depth=4, seed=3, resolution=(64, 64), world=world)
    a = render(scene, cam, spp=K * n, denoise="variance", variance_batches=K, **kw)
    acc = Accumulator(scene, cam, moments=True, **kw)
    acc.add(n).add(n)
    # below MIN_MOMENT_BATCHES the spatial estimate is used
    assert acc.batches == 2 < D.MIN_MOMENT_BATCHES
    assert np.array_equal(bits(acc.denoised(mode="variance")), bits(D.denoise_variance(acc.mean(), acc.features())))
    acc.add(0).add(n).add(n)
    b = acc.denoised(mode="variance")
    assert acc.samples == K * n and acc.batches == K
    assert np.array_equal(bits(a), bits(b)) and np.isfinite(a).all()
    sums, feat, state = render_batches(scene, cam, spp=K * n, depth=4, variance_batches=K, seed=3, resolution=(64, 64),
                                       world=world)
    assert np.array_equal(bits(state), bits(acc.moments_state)) and np.array_equal(bits(sums), bits(acc.sums()))
    assert np.array_equal(bits(feat), bits(acc.features()))
    assert (state[..., 0] == K).all()
    assert np.array_equal(bits(a), bits(D.denoise_variance(acc.mean(), feat, variance=state[..., 3])))
    assert not np.array_equal(a, D.denoise_variance(acc.mean(), feat))   # not the spatial estimate's image
    assert np.array_equal(bits(acc.noise_map()), bits(np.sqrt(state[..., 3]))) and (state[..., 3] > 0).mean() > 0.9
    # the state's mean against lum of the demodulated total mean.  In exact arithmetic both are the mean of
    # the K batch luminances l_j.  All terms are non-negative, so rounding errors stay relative: Welford's
    # mean makes 3 roundings per batch (3 K), each l_j 7 (/ n, / a, 5 in lum), the total mean K adds and
    # again 7: (4 K + 14) eps relative to max_j l_j <= K * mean.
    I, _, _, _, _, hit, bad, _ = R.prepass(acc.mean(), feat, D.EPS_A)
    l_total = V.lum(I).astype(np.float64)
    tol = (4 * K + 14) * EPS32 * K * np.abs(l_total)
    assert not bad.any()
    assert np.all(np.abs(state[..., 1] - l_total) <= tol), float(np.max(np.abs(state[..., 1] - l_total) / np.maximum(tol, 1e-300)))
    # unequal batches are refused, and the sums differ from render()'s only in the last bits
    with pytest.raises(ValueError, match="equal batches"):
        acc.add(3)
    plain = render(scene, cam, spp=K * n, **kw)
    assert np.allclose(acc.mean(), plain, rtol=K * n * EPS32, atol=0)
    # save / load carry the moments; a file without them loads as moments=False
    acc.save(tmp_path / "m.npz")
    back = Accumulator.load(tmp_path / "m.npz", scene, cam, world=world)
    assert back.moments and back.batch_spp == n and back.batches == K
    assert np.array_equal(bits(back.moments_state), bits(state))
    assert np.array_equal(bits(back.denoised(mode="variance")), bits(a))
    old = Accumulator(scene, cam, **kw).add(K * n)
    old.save(tmp_path / "p.npz")
    assert sorted(np.load(tmp_path / "p.npz").files) == sorted(
        ["slots", "samples", "seed", "depth", "resolution", "tile", "flags", "camera", "scene_sha"])
    assert not Accumulator.load(tmp_path / "p.npz", scene, cam, world=world).moments
    assert np.array_equal(bits(old.mean()), bits(plain))


def test_command_line_writes_the_variance_it_used(tmp_path):
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import render_batches
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    from pyrenderer_amd.main import main
    aov = str(tmp_path / "aov")
    img = main(["--resolution", "32", "24", "--depth", "4", "--seed", "5", "--samples", "8", "--denoise",
                "--denoise-mode", "variance", "--variance-batches", "4", "--aov", aov, "--out", str(tmp_path / "m.png")])
    assert sorted(os.listdir(aov)) == ["albedo.png", "depth.npy", "normal.png", "variance.npy"]
    scene, cam = read_file(CORNELL_JSON)
    sums, feat, state = render_batches(scene, cam, spp=8, depth=4, variance_batches=4, seed=5, resolution=(32, 24))
    var = np.load(os.path.join(aov, "variance.npy"))
    _, _, _, _, _, hit, bad, _ = R.prepass(sums / F32(8), feat, D.EPS_A)
    assert var.shape == (32, 24) and var.dtype == F32
    assert np.array_equal(bits(var), bits(M.given(state[..., 3], hit & ~bad))) and var.any()
    assert np.array_equal(bits(img), bits(D.denoise_variance(sums / F32(8), feat, variance=state[..., 3])))
    # progressive: every pass is a batch
    prog = main(["--resolution", "32", "24", "--depth", "4", "--seed", "5", "--samples", "8", "--interval", "2",
                 "--denoise", "--denoise-mode", "variance", "--variance-batches", "4", "--out", ""])
    assert np.array_equal(bits(prog), bits(img))


def test_command_line_render_and_accumulator_agree_on_ragged_tiles(cornell):
    """Cornell 72 x 40 (two 64-pixel tiles, one ragged in x, both in y), depth 4, 8 spp, seed 3: the command
    line, render() and the matching Accumulator route return the same bits, unfiltered and in every filter mode."""
    from pyrenderer_amd.core.tracing import Accumulator, build_world, render
    from pyrenderer_amd.main import main
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    kw = dict(depth=4, seed=3, resolution=(72, 40), world=world)
    argv = ["--resolution", "72", "40", "--depth", "4", "--seed", "3", "--samples", "8", "--out", ""]
    var = ["--denoise", "--denoise-mode", "variance"]
    plain = Accumulator(scene, cam, **kw).add(3).add(5)
    batched = Accumulator(scene, cam, moments=True, **kw)
    for _ in range(4):
        batched.add(2)
    images = []
    for switches, render_kw, route in (
            ([], dict(), plain.mean),
            (["--denoise"], dict(denoise=True), plain.denoised),
            (var, dict(denoise="variance"), lambda: plain.denoised(mode="variance")),
            (var + ["--variance-batches", "4"], dict(denoise="variance", variance_batches=4),
             lambda: batched.denoised(mode="variance"))):
        want = render(scene, cam, spp=8, **render_kw, **kw)
        assert want.shape == (72, 40, 3) and np.isfinite(want).all() and want[64:, :].any() and want[:, 39].any()
        assert np.array_equal(bits(main(argv + switches)), bits(want)), switches
        assert np.array_equal(bits(route()), bits(want)), switches
        images.append(want)
    for i in range(4):   # four different images: the equalities above are not one image four times
        for j in range(i):
            assert not np.array_equal(images[i], images[j]), (i, j)


# ----------------------------------------------------------------- quality ----

# RMSE(denoised) / RMSE(noisy) against the 4096-spp render, measured on the MI355X with the default
# parameters and the variance of K batch means (profiles/denoise_mom_sweep.txt, the
# 128^2 columns of the default row).  The margin rule of test_gpu_denoise.test_it_denoises: sqrt(rho).
RHO = {("cornell", 8, 4): 0.4340, ("specular", 8, 4): 0.4889, ("cornell", 64, 8): 0.5332, ("specular", 64, 8): 0.6597}


@pytest.mark.parametrize("which,spp,K", sorted(RHO))
def test_it_denoises(which, spp, K):
    from pyrenderer_amd.core.tracing import render_batches
    from pyrenderer_amd.denoise import denoise_variance
    scene, cam, world, ref = reference(which)
    sums, feat, state = render_batches(scene, cam, spp=spp, depth=8, variance_batches=K, seed=2, resolution=(128, 128),
                                       world=world)
    noisy = sums / F32(spp)
    den = denoise_variance(noisy, feat, variance=state[..., 3])
    e_noisy, e_den = rmse(noisy, ref), rmse(den, ref)
    print(f"moments quality {which} {spp} spp K {K}: rmse noisy {e_noisy:.6f} denoised {e_den:.6f} "
          f"ratio {e_den / e_noisy:.4f}")
    assert np.isfinite(den).all()
    assert e_den < e_noisy, (e_den, e_noisy)
    assert e_den / e_noisy <= np.sqrt(RHO[(which, spp, K)]), (e_den / e_noisy, RHO[(which, spp, K)])

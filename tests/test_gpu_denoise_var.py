"""The variance-guided a-trous mode on the GPU: prt_denoise_var against the NumPy restatement bit
for bit (image and variance estimate), the device entry point, the public API and the quality gain."""
import os

import numpy as np
import pytest

import atrous_var_ref as V
from denoise_cases import bits, hostile_inputs, reference, rmse

pytestmark = pytest.mark.gpu

F32 = np.float32
# non-default parameters for the bit-identity cases, so every term of the weight is at work
PAR = dict(sigma_l=1.5, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3, eps_l=3e-3)


# 3 x 7 is narrower than the 7 x 7 window and the 5 x 5 stencil; 70 x 130 crosses the 64-lane and
# 4-wave block edges and its step-16 stencil reaches 32 px
_CASES = [(1, 1, 5), (3, 7, 5), (33, 17, 4), (70, 130, 5)]


@pytest.fixture(scope="module")
def restated():
    """Inputs and the restatement's outputs of every shape, computed once and left unchanged."""
    out = {}
    for W, H, n in _CASES:
        C, F, bad = hostile_inputs(W, H, 200 + W, "halves")
        out[(W, H)] = (C, F, bad, n) + V.atrous_var(C, F, n, **PAR)
    return out


@pytest.mark.parametrize("W,H", [c[:2] for c in _CASES])
def test_filter_equals_the_restatement_bit_for_bit(restated, W, H):
    from pyrenderer_amd.denoise import denoise_variance
    C, F, bad, n, want, want_var = restated[(W, H)]
    got, var = denoise_variance(C, F, iterations=n, return_variance=True, **PAR)
    again, var2 = denoise_variance(C, F, iterations=n, return_variance=True, **PAR)
    assert np.array_equal(bits(got), bits(again)) and np.array_equal(bits(var), bits(var2))
    assert var.shape == (W, H) and var.dtype == F32
    diff = np.argwhere(bits(var) != bits(want_var))
    assert len(diff) == 0, ("variance", len(diff), diff[:5])
    diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
    assert len(diff) == 0, ("image", len(diff), diff[:5])
    assert np.array_equal(bits(got), bits(denoise_variance(C, F, iterations=n, **PAR)))   # without out_var
    ok = np.ones((W, H), bool)
    for x, y in bad:
        ok[x, y] = False
        assert np.array_equal(bits(got[x, y]), bits(C[x, y])) and var[x, y] == 0
    assert np.isfinite(got[ok]).all() and np.isfinite(var).all() and (var >= 0).all()
    miss = ~(F[..., 7] > 0)
    if W * H > 1:
        assert miss.any() and (~miss).any()
    assert np.array_equal(bits(got[miss]), bits(C[miss])) and not var[miss].any()
    if W * H > 100:   # the filter did something, and the estimate is at work
        assert np.mean(np.any(got[ok & ~miss] != C[ok & ~miss], axis=-1)) > 0.6
        assert np.mean(var[ok & ~miss] > 0) > 0.6


@pytest.mark.parametrize("n", [0, 1, 8])
def test_iteration_counts_at_the_ends_of_the_range(restated, n):
    from pyrenderer_amd.denoise import denoise_variance
    C, F, _, _, _, want_var = restated[(33, 17)]
    got, var = denoise_variance(C, F, iterations=n, return_variance=True, **PAR)
    assert np.array_equal(bits(got), bits(V.atrous_var(C, F, n, **PAR)[0]))
    assert np.array_equal(bits(var), bits(want_var))   # the estimate precedes the passes


def test_outputs_are_finite_at_the_stated_bound():
    """Demodulated radiance of magnitude 2^126, albedo 1 (include/prt.h): finite, and the restatement's bits."""
    W, H = 9, 8
    rng = np.random.default_rng(10)
    C = (rng.choice([-1.0, 1.0], (W, H, 3)) * 2.0 ** 126).astype(F32)
    C[2, 3] = (2.0 ** 126, 1.0, -3.0)
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = 1.0
    F[..., 5] = 1.0
    F[..., 6] = 4.0
    F[..., 7] = 1.0
    from pyrenderer_amd.denoise import denoise_variance
    for eps_l in (2.0 ** 125, 1e-3):
        got, var = denoise_variance(C, F, iterations=5, eps_l=eps_l, return_variance=True)
        want, want_var = V.atrous_var(C, F, 5, eps_l=eps_l)
        assert np.isfinite(got).all() and not var.any()
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(var), bits(want_var))


@pytest.mark.parametrize("with_var", [True, False])
def test_device_entry_point_on_a_side_stream(restated, with_var):
    import torch
    from pyrenderer_amd import denoise as D
    C, F, _, n, want, want_var = restated[(70, 130)]
    W, H = C.shape[:2]
    dev = torch.device("cuda:0")
    d_c, d_f = torch.from_numpy(C).to(dev), torch.from_numpy(F).to(dev)
    d_out = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    d_var = torch.full((W, H), -1.0, dtype=torch.float32, device=dev)
    need = D.work_bytes_variance(W, H)
    assert need > 0
    d_work = torch.empty(need, dtype=torch.uint8, device=dev)   # exactly the bytes asked for
    assert d_work.data_ptr() % 16 == 0
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    D.denoise_variance_device(d_c.data_ptr(), d_f.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(), need,
                              d_out_var_ptr=d_var.data_ptr() if with_var else None, iterations=n,
                              stream_ptr=stream.cuda_stream, **PAR)
    stream.synchronize()
    got = d_out.cpu().numpy()
    host, host_var = D.denoise_variance(C, F, iterations=n, return_variance=True, **PAR)
    assert np.array_equal(bits(got), bits(host)) and np.array_equal(bits(got), bits(want))
    if with_var:
        assert np.array_equal(bits(d_var.cpu().numpy()), bits(host_var))
        assert np.array_equal(bits(host_var), bits(want_var))
    else:
        assert (d_var.cpu().numpy() == -1.0).all()   # left alone


# ----------------------------------------------------------------- quality ----

# RMSE(denoised) / RMSE(noisy) against the 4096-spp render, measured on the MI355X with the default
# parameters of the variance-guided mode (the columns of the chosen row of
# profiles/denoise_var_sweep.txt, which are these very frames).  The 8-spp tests allow sqrt(rho), the
# margin rule of test_gpu_denoise.test_it_denoises; the 64-spp specular frame must simply improve.
RHO = {("cornell", 8): 0.4719, ("specular", 8): 0.5139}


@pytest.fixture(scope="module")
def frames():
    """Per scene: the world, the 4096-spp reference (seed 1) and the one-sample features (seed 2) at 128^2."""
    from pyrenderer_amd.denoise import features
    out = {}
    for which in ("cornell", "specular"):
        scene, cam, world, ref = reference(which)
        feat = features(scene, cam, resolution=(128, 128), samples=1, seed=2, world=world)
        out[which] = (scene, cam, world, ref, feat)
    return out


@pytest.mark.parametrize("which,spp", [("cornell", 8), ("specular", 8), ("specular", 64)])
def test_it_denoises(frames, which, spp):
    from pyrenderer_amd.core.tracing import render
    from pyrenderer_amd.denoise import denoise_variance
    scene, cam, world, ref, feat = frames[which]
    noisy = render(scene, cam, spp=spp, depth=8, seed=2, resolution=(128, 128), world=world)
    den = denoise_variance(noisy, feat)
    e_noisy, e_den = rmse(noisy, ref), rmse(den, ref)
    print(f"variance-guided quality {which} {spp} spp: rmse noisy {e_noisy:.6f} denoised {e_den:.6f} "
          f"ratio {e_den / e_noisy:.4f}")
    assert np.isfinite(den).all()
    assert e_den < e_noisy, (e_den, e_noisy)
    if (which, spp) in RHO:
        assert e_den / e_noisy <= np.sqrt(RHO[(which, spp)]), (e_den / e_noisy, RHO[(which, spp)])


# -------------------------------------------------------------- public API ----

def test_public_entry_points_agree(cornell):
    from pyrenderer_amd.core.tracing import Accumulator, build_world, render
    from pyrenderer_amd.denoise import denoise, denoise_variance, features
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    kw = dict(depth=4, seed=3, resolution=(64, 64), world=world)
    plain = render(scene, cam, spp=4, **kw)
    feat = features(scene, cam, resolution=(64, 64), samples=1, seed=3, world=world)
    a = render(scene, cam, spp=4, denoise="variance", **kw)
    b = denoise_variance(plain, feat)
    acc = Accumulator(scene, cam, **kw)
    c = acc.add(4).denoised(mode="variance")
    assert np.array_equal(bits(acc.mean()), bits(plain))
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    assert not np.array_equal(a, plain) and np.isfinite(a).all()
    # parameters reach the filter, and the fixed mode is what it was
    assert np.array_equal(bits(acc.denoised(mode="variance", sigma_l=1.0)), bits(denoise_variance(plain, feat, sigma_l=1.0)))
    fixed = render(scene, cam, spp=4, denoise=True, **kw)
    assert np.array_equal(bits(fixed), bits(denoise(plain, feat)))
    assert np.array_equal(bits(fixed), bits(acc.denoised())) and np.array_equal(bits(fixed), bits(acc.denoised(mode="fixed")))
    assert not np.array_equal(fixed, a)
    with pytest.raises(ValueError):
        acc.denoised(mode="nonsense")


def test_command_line_writes_the_variance_aov(tmp_path):
    """--denoise --denoise-mode variance --aov DIR: the feature buffers and variance.npy; the fixed mode writes none."""
    from pyrenderer_amd.main import main
    common = ["--resolution", "32", "24", "--depth", "4", "--seed", "5", "--samples", "2", "--denoise"]
    aov, aov_fixed = str(tmp_path / "aov"), str(tmp_path / "aov_fixed")
    main(common + ["--denoise-mode", "variance", "--aov", aov, "--out", str(tmp_path / "v.png")])
    main(common + ["--aov", aov_fixed, "--out", str(tmp_path / "f.png")])
    assert sorted(os.listdir(aov)) == ["albedo.png", "depth.npy", "normal.png", "variance.npy"]
    assert sorted(os.listdir(aov_fixed)) == ["albedo.png", "depth.npy", "normal.png"]
    var = np.load(os.path.join(aov, "variance.npy"))
    assert var.shape == (32, 24) and var.dtype == F32 and np.isfinite(var).all() and (var >= 0).all() and var.any()
    assert open(tmp_path / "v.png", "rb").read() != open(tmp_path / "f.png", "rb").read()

"""The NumPy restatement of the variance-guided a-trous mode (tests/atrous_var_ref.py), pinned on
its own: the GPU tests compare prt_denoise_var against it bit for bit, so its properties are checked
without a GPU."""
import numpy as np

import atrous_ref as R
import atrous_var_ref as V

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _frame(W, H, seed=0):
    """Colour and features of an all-hit frame with unit normals and a depth ramp."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(0.0, 2.0, (W, H, 3)).astype(F32)
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = rng.uniform(0.05, 1.0, (W, H, 3))
    n = rng.normal(size=(W, H, 3))
    F[..., 3:6] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    F[..., 6] = 2.0 + 0.01 * np.arange(W)[:, None] + 0.02 * np.arange(H)[None, :]
    F[..., 7] = 1.0
    return C, F


def _flat(W, H, albedo=0.5):
    """Features of one flat surface facing the camera."""
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = albedo
    F[..., 5] = 1.0
    F[..., 6] = 4.0
    F[..., 7] = 1.0
    return F


def test_constant_frame_has_variance_zero_and_is_a_fixed_point():
    """Equal colours, normals and depth.  Every estimate weight is exactly 1 (w_n = 1, x_z = 0), and the
    demodulated value 0.75 / 0.5 = 1.5 has luminance exactly 1.5: the sums k * 1.5 and k * 2.25, k <= 49,
    are exact, so mu * mu equals m2 / sw and the variance is exactly 0.  With sd = 0 and equal
    luminances every pass weight is h, and the normalised sum returns the colour up to rounding."""
    W, H = 13, 9
    C = np.full((W, H, 3), 0.75, F32)
    out, est, last = V.atrous_var(C, _flat(W, H), 5, return_final_variance=True)
    assert est.dtype == F32 and est.shape == (W, H)
    assert not est.any() and not last.any()
    assert np.max(np.abs(out - C)) <= 4 * np.spacing(F32(0.75))
    # a constant colour that is not grey: the estimate is 0 up to the rounding of its sums
    C2 = np.empty((W, H, 3), F32)
    C2[...] = (0.3, 0.9, 0.55)
    out2, est2 = V.atrous_var(C2, _flat(W, H, 0.7), 5)
    l2 = float(V.lum(C2[0, 0] / F32(0.7)))
    assert est2.max() <= 49 * 4 * float(np.spacing(F32(l2 * l2)))
    assert np.max(np.abs(out2 - C2)) <= 4 * np.spacing(F32(0.9))


def test_all_miss_frame_is_returned_bit_for_bit():
    C, F = _frame(19, 11, 1)
    F[...] = 0.0
    out, est = V.atrous_var(C, F, 5)
    assert out.dtype == F32 and np.array_equal(_bits(out), _bits(C))
    assert not est.any()
    C2, F2 = _frame(19, 11, 2)
    F2[..., 7] = 0.0   # leftover feature values on the missed pixels: a miss is never filtered
    out2, est2 = V.atrous_var(C2, F2, 3)
    assert np.array_equal(_bits(out2), _bits(C2)) and not est2.any()


def test_zero_iterations_is_the_demodulation_round_trip():
    """n = 0 returns (C / a) * a, exactly what the fixed filter's n = 0 returns; the estimate is still made."""
    C, F = _frame(33, 17, 3)
    F[:4, :, 0:3] = 1e-4   # albedo below eps_a
    out, est = V.atrous_var(C, F, 0, eps_a=1e-2)
    assert np.array_equal(_bits(out), _bits(R.atrous(C, F, 0, eps_a=1e-2)))
    d = np.abs(out.view(np.int32).astype(np.int64) - C.view(np.int32).astype(np.int64))
    assert d.max() <= 2
    assert np.array_equal(_bits(est), _bits(V.atrous_var(C, F, 3, eps_a=1e-2)[1])) and est.max() > 0


def test_orthogonal_half_planes_do_not_exchange_a_bit():
    """Two half-planes with orthogonal normals: w_n is exactly 0 across the edge, in the estimate and
    in every pass, so colour and variance sums take nothing from the other side.  The one quantity
    that looks across is the 3 x 3 variance prefilter, whose taps are class-tested but not
    normal-weighted: the column next to the edge sees the other side's variance in its sd.
    So: (a) the estimate exchanges not one bit; (b) with eps_l so large that it absorbs sigma_l * sd
    (den == eps_l in f32) the whole multi-pass image exchanges not one bit; (c) with the luminance term
    at work, one pass changes no bit outside the column next to the edge."""
    W, H = 24, 20
    C, F = _frame(W, H, 4)
    F[:W // 2, :, 3:6] = (1.0, 0.0, 0.0)
    F[W // 2:, :, 3:6] = (0.0, 1.0, 0.0)
    F[..., 6] = 3.0
    F[..., 0:3] = 0.5
    C2 = C.copy()
    C2[W // 2:] = np.random.default_rng(5).uniform(0.0, 50.0, C2[W // 2:].shape).astype(F32)
    big = dict(sigma_l=1.0, eps_l=1e30)
    out1, est1 = V.atrous_var(C, F, 4, **big)
    out2, est2 = V.atrous_var(C2, F, 4, **big)
    assert np.array_equal(_bits(est1[:W // 2]), _bits(est2[:W // 2]))
    assert not np.array_equal(est1[W // 2:], est2[W // 2:])
    assert np.array_equal(_bits(out1[:W // 2]), _bits(out2[:W // 2]))
    assert not np.array_equal(out1[W // 2:], out2[W // 2:])
    assert out1[:W // 2].std() < 0.7 * C[:W // 2].std()   # the filter did mix within a side
    one = V.atrous_var(C, F, 1, sigma_l=2.0)[0]
    two = V.atrous_var(C2, F, 1, sigma_l=2.0)[0]
    assert np.array_equal(_bits(one[:W // 2 - 1]), _bits(two[:W // 2 - 1]))
    assert np.any(one[:W // 2 - 1] != C[:W // 2 - 1])


def test_non_finite_pixels_are_set_aside():
    C, F = _frame(12, 10, 6)
    F[..., 3:6] = (0.0, 0.0, 1.0)
    C[3, 4, 1] = np.nan
    C[8, 2, 0] = np.inf
    out, est = V.atrous_var(C, F, 3)
    mask = np.ones((12, 10), bool)
    for x, y in ((3, 4), (8, 2)):
        assert np.array_equal(_bits(out[x, y]), _bits(C[x, y])) and est[x, y] == 0
        mask[x, y] = False
    assert np.isfinite(out[mask]).all() and np.isfinite(est).all() and (est[mask] > 0).all()


def test_non_finite_features_are_set_aside_too():
    C, F = _frame(14, 12, 7)
    F[..., 3:6] = (0.0, 0.0, 1.0)
    F[5, 5, 6] = np.nan
    F[9, 3, 3] = np.inf
    F[2, 8, 0] = -np.inf
    out, est = V.atrous_var(C, F, 4)
    mask = np.ones((14, 12), bool)
    for x, y in ((5, 5), (9, 3), (2, 8)):
        assert np.array_equal(_bits(out[x, y]), _bits(C[x, y])) and est[x, y] == 0
        mask[x, y] = False
    assert np.isfinite(out[mask]).all() and np.isfinite(est).all()
    assert np.any(out[4, 5] != C[4, 5]) and np.any(out[5, 6] != C[5, 6])


def test_noise_scale_equivariance():
    """Colour and eps_l times 4: every luminance, standard deviation and denominator is scaled by an
    exact power of two, so every weight keeps its bits, the output is exactly 4 times and the
    variance estimate exactly 16 times the original.  The fixed-sigma_c filter has no such property."""
    C, F = _frame(21, 18, 8)
    F[..., 3:6] = np.where(np.arange(21)[:, None, None] < 12, (0.0, 0.0, 1.0), (0.0, 0.6, 0.8))
    par = dict(sigma_l=2.0, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3)
    out1, est1 = V.atrous_var(C, F, 4, eps_l=1e-3, **par)
    out4, est4 = V.atrous_var(F32(4.0) * C, F, 4, eps_l=F32(4.0) * F32(1e-3), **par)
    assert np.array_equal(_bits(out4), _bits(F32(4.0) * out1))
    assert np.array_equal(_bits(est4), _bits(F32(16.0) * est1))
    assert np.any(out1 != C) and est1.min() > 0
    fixed1 = R.atrous(C, F, 4, sigma_c=0.25)
    fixed4 = R.atrous(F32(4.0) * C, F, 4, sigma_c=0.25)
    assert not np.array_equal(_bits(fixed4), _bits(F32(4.0) * fixed1))


def test_two_noise_levels():
    """Left half: noise amplitude 0.05, right half: 0.6, around the same mean.  Uniform noise of
    amplitude a has variance a^2 / 3, so the true ratio of the variances is 144; the estimate's medians
    must be at least 50 apart, and the filter must lower the variance in both halves."""
    W, H = 48, 40
    rng = np.random.default_rng(9)
    amp = np.where(np.arange(W)[:, None, None] < W // 2, 0.05, 0.6)
    C = (1.0 + amp * rng.uniform(-1.0, 1.0, (W, H, 3))).astype(F32)
    F = _flat(W, H, 1.0)
    out, est = V.atrous_var(C, F, 5)
    left, right = slice(0, W // 2 - 4), slice(W // 2 + 4, W)   # clear of the windows that straddle the seam
    ratio = np.median(est[right]) / np.median(est[left])
    assert ratio >= 50, ratio
    lum_in, lum_out = V.lum(C), V.lum(out)
    for side in (left, right):
        assert lum_out[side].var() < 0.25 * lum_in[side].var(), (lum_out[side].var(), lum_in[side].var())
    # and the estimate is about the variance of the luminance it saw
    assert 0.5 < np.median(est[right]) / lum_in[right].var() < 2.0


def test_outputs_are_finite_at_the_stated_bound():
    """Demodulated radiance of magnitude 2^126 with albedo 1 (prt_denoise.h): l * l overflows, the
    estimate's guard turns that into variance 0, and every colour comes out finite."""
    W, H = 9, 8
    rng = np.random.default_rng(10)
    C = (rng.choice([-1.0, 1.0], (W, H, 3)) * 2.0 ** 126).astype(F32)
    C[2, 3] = (2.0 ** 126, 1.0, -3.0)
    # eps_l of the colours' own magnitude: the weights between unequal pixels are not 0 and the sums mix them
    out, est, last = V.atrous_var(C, _flat(W, H, 1.0), 5, eps_l=2.0 ** 125, return_final_variance=True)
    assert np.isfinite(out).all() and np.isfinite(est).all() and np.isfinite(last).all()
    assert not est.any()
    assert np.mean(np.any(out != C, axis=-1)) > 0.5
    # with the default floor every weight between unequal pixels is 0: still finite
    assert np.isfinite(V.atrous_var(C, _flat(W, H, 1.0), 5)[0]).all()

"""The NumPy restatement of the sample-moments kernels (tests/moments_ref.py) against float64 and
against its own properties; no GPU."""
import numpy as np

import atrous_var_ref as V
import moments_ref as M

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _scene(W, H, K, seed, n=4.0):
    """K frames of radiance sums over n samples, with features: hit pixels with albedo in [0.2, 1], a few
    below eps_a, a block of misses."""
    rng = np.random.default_rng(seed)
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = rng.uniform(0.2, 1.0, (W, H, 3))
    F[..., 5] = 1.0
    F[..., 6] = 2.0
    F[..., 7] = 1.0
    F[0, 0, 0:3] = (1e-3, 0.0, 5e-3)
    F[W // 2:, H // 2:] = 0.0
    S = (n * F[None, ..., 0:3].clip(0.1, None) * rng.uniform(0.5, 1.5, (K, W, H, 3))).astype(F32)
    S[:, W // 2:, H // 2:] = (n * rng.uniform(0.5, 1.5, (K, W - W // 2, H - H // 2, 3))).astype(F32)
    return S, F, F32(n)


def _lum_of_frames(S, F, n, eps_a):
    """The batch luminances as the kernel forms them, f32."""
    hit = F[..., 7] > 0
    a = np.fmax(F[..., 0:3], F32(eps_a))
    c = (S / n).astype(F32)
    I = np.where(hit[None, ..., None], c / a[None], c).astype(F32)
    return V.lum(I).astype(F32)


def test_variance_of_the_mean_agrees_with_float64_two_pass():
    for K in (2, 4, 8, 64):
        S, F, n = _scene(9, 7, K, 40 + K)
        st = M.moments_add(np.zeros((9, 7, 4), F32), S, n, F, 1e-2)
        l = _lum_of_frames(S, F, n, 1e-2).astype(np.float64)
        mean = l.mean(axis=0)
        m2 = ((l - mean) ** 2).sum(axis=0)
        want = m2 / (K - 1) / K
        # Welford's update makes six f32 roundings per frame (d, d / k', mean', l - mean', the product, the
        # sum); over K frames their effect on M2 is bounded by the condition number of the sample variance,
        # kappa = |l|_2 / sqrt(M2) (Chan, Golub, LeVeque 1983): relative error <= 6 K kappa eps, plus two
        # roundings for the divisions by k - 1 and k
        kappa = np.sqrt((l ** 2).sum(axis=0) / m2)
        tol = (6 * K * kappa + 2) * EPS32
        assert np.all(st[..., 0] == K)
        assert np.all(np.abs(st[..., 3] - want) <= tol * want), float(np.max(np.abs(st[..., 3] - want) / (tol * want)))
        assert np.all(np.abs(st[..., 1] - mean) <= 2 * K * EPS32 * np.abs(l).max(axis=0))
        assert st.dtype == F32 and (st[..., 3] > 0).all()


def test_one_call_equals_two_calls_bit_for_bit():
    S, F, n = _scene(6, 5, 7, 3)
    zero = np.zeros((6, 5, 4), F32)
    whole = M.moments_add(zero, S, n, F)
    for cut in (1, 3, 6):
        split = M.moments_add(M.moments_add(zero, S[:cut], n, F), S[cut:], n, F)
        assert np.array_equal(_bits(whole), _bits(split)), cut
    assert not zero.any()   # the input state is left alone


def test_a_non_finite_frame_is_skipped():
    S, F, n = _scene(6, 5, 5, 4)
    zero = np.zeros((6, 5, 4), F32)
    bad = S.copy()
    bad[2, 1, 1, 0] = np.nan      # a hit pixel
    bad[2, 4, 4, 2] = np.inf      # a miss pixel
    bad[2, 0, 0] = 3e38           # finite over an albedo below eps_a: overflows in the demodulation
    got = M.moments_add(zero, bad, n, F)
    without = M.moments_add(zero, np.delete(S, 2, axis=0), n, F)
    full = M.moments_add(zero, S, n, F)
    for x, y in ((1, 1), (4, 4), (0, 0)):
        assert got[x, y, 0] == 4
        assert np.array_equal(_bits(got[x, y]), _bits(without[x, y]))
    rest = np.ones((6, 5), bool)
    rest[1, 1] = rest[4, 4] = rest[0, 0] = False
    assert np.array_equal(_bits(got[rest]), _bits(full[rest])) and np.isfinite(got).all()


def test_one_batch_has_variance_zero():
    S, F, n = _scene(4, 3, 1, 5)
    st = M.moments_add(np.zeros((4, 3, 4), F32), S, n, F)
    assert np.all(st[..., 0] == 1) and not st[..., 2].any() and not st[..., 3].any()
    assert np.array_equal(_bits(st[..., 1]), _bits(_lum_of_frames(S, F, n, 1e-2)[0]))   # 0 + l / 1


def test_state_is_finite_at_the_stated_bound_and_guarded_beyond():
    """|l| <= 2^62 for up to 8 frames (include/prt.h): every product d * (l - mean') is at most 2^126 and
    M2 at most 8 * 2^124.  Beyond the bound M2 overflows and var_mean is stored as 0."""
    W, H, K = 3, 2, 8
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = 1.0
    F[..., 7] = 1.0
    F[2, 1] = 0.0
    sign = np.where(np.arange(K) % 2 == 0, 1.0, -1.0)[:, None, None, None]
    S = (sign * 2.0 ** 62 * np.ones((K, W, H, 3))).astype(F32)
    st = M.moments_add(np.zeros((W, H, 4), F32), S, 1.0, F)
    assert np.isfinite(st).all() and (st[..., 0] == K).all() and (st[..., 3] > 0).all()
    assert st[..., 2].max() >= 2.0 ** 126
    over = M.moments_add(np.zeros((W, H, 4), F32), S * F32(4.0), 1.0, F)
    assert np.isinf(over[..., 2]).all() and not over[..., 3].any() and np.isfinite(over[..., 0:2]).all()


def test_given_variance_sanitises_and_replaces_only_the_estimate():
    rng = np.random.default_rng(6)
    W, H = 9, 8
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = rng.uniform(0.2, 1.0, (W, H, 3))
    F[..., 5] = 1.0
    F[..., 6] = 2.0 + 0.01 * np.arange(W)[:, None]
    F[..., 7] = 1.0
    F[0:2, 0:2] = 0.0
    C = (F[..., 0:3] * rng.uniform(0.7, 1.3, (W, H, 3))).astype(F32)
    C[3, 3, 0] = np.nan
    out, est = V.atrous_var(C, F, 3)
    again, used = M.atrous_var_given(C, F, est, 3)
    assert np.array_equal(_bits(out), _bits(again)) and np.array_equal(_bits(est), _bits(used))
    iv = rng.uniform(0.0, 0.1, (W, H)).astype(F32)
    dirty = iv.copy()
    clean = iv.copy()
    for (x, y), v in (((4, 4), np.nan), ((5, 5), np.inf), ((6, 6), -1.0), ((7, 7), -np.inf)):
        dirty[x, y] = v
        clean[x, y] = 0.0
    a, ua = M.atrous_var_given(C, F, dirty, 2)
    b, ub = M.atrous_var_given(C, F, clean, 2)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(ua), _bits(ub))
    assert not ua[0:2, 0:2].any() and ua[3, 3] == 0 and np.isfinite(ua).all()
    mz = iv.copy()
    mz[4, 4] = -0.0
    assert _bits(M.atrous_var_given(C, F, mz, 0)[1])[4, 4] == 0x80000000   # a -0 is passed on

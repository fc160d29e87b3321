"""The NumPy restatement of the a-trous filter (tests/atrous_ref.py), pinned on its own: the GPU
tests compare prt_denoise against it bit for bit, so its properties are checked without a GPU."""
import numpy as np

import atrous_ref as R

F32 = np.float32


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


def test_e_is_one_at_zero_and_decreasing():
    assert R.e16(F32(0.0)) == F32(1.0)
    x = np.concatenate([np.linspace(0.0, 8.0, 4001), np.geomspace(8.0, 1e6, 400)]).astype(F32)
    e = R.e16(x)
    assert e.dtype == F32
    assert np.all(np.diff(e) <= 0) and np.all(np.diff(e[:2000]) < 0)
    assert np.all((e > 0) | (x > 1e3)) and np.all(e <= 1)
    # the stand-in follows exp(-x) where the weights matter
    assert np.max(np.abs(e[:1001] - np.exp(-x[:1001].astype(np.float64)))) < 0.05


def test_all_miss_frame_is_returned_bit_for_bit():
    C, F = _frame(19, 11, 1)
    F[..., 7] = 0.0
    F[..., 0:6] = 0.0
    F[..., 6] = 0.0
    out = R.atrous(C, F, 5)
    assert out.dtype == F32 and np.array_equal(out.view(np.uint32), C.view(np.uint32))
    # also with leftover feature values on the missed pixels: a miss is never filtered
    C2, F2 = _frame(19, 11, 2)
    F2[..., 7] = 0.0
    assert np.array_equal(R.atrous(C2, F2, 3).view(np.uint32), C2.view(np.uint32))


def test_zero_iterations_is_the_demodulation_round_trip():
    """n = 0 returns (C / a) * a: one division and one multiplication, each within half an ulp, so
    the result is within 2 ulp of C (1.5 ulp in exact terms; 2 in whole units of the last place)."""
    C, F = _frame(33, 17, 3)
    F[:4, :, 0:3] = 1e-4   # albedo below eps_a: divided and multiplied by eps_a
    out = R.atrous(C, F, 0, eps_a=1e-2)
    ulp = np.spacing(np.abs(C))
    assert np.all(np.abs(out.astype(np.float64) - C) <= 2.0 * ulp)
    d = np.abs(out.view(np.int32).astype(np.int64) - C.view(np.int32).astype(np.int64))
    assert d.max() <= 2


def test_orthogonal_half_planes_do_not_exchange_a_bit():
    """Two half-planes with orthogonal normals: w_n is exactly 0 across the edge, so changing the
    colours of one side leaves the other side's output bits unchanged."""
    W, H = 24, 20
    C, F = _frame(W, H, 4)
    F[:W // 2, :, 3:6] = (1.0, 0.0, 0.0)
    F[W // 2:, :, 3:6] = (0.0, 1.0, 0.0)
    F[..., 6] = 3.0   # same depth: only the normal separates the sides
    F[..., 0:3] = 0.5   # one albedo: the smoothing shows in the output itself
    out1 = R.atrous(C, F, 4, sigma_c=1e3)
    C2 = C.copy()
    C2[W // 2:] = np.random.default_rng(5).uniform(0.0, 50.0, C2[W // 2:].shape).astype(F32)
    out2 = R.atrous(C2, F, 4, sigma_c=1e3)
    assert np.array_equal(out1[:W // 2].view(np.uint32), out2[:W // 2].view(np.uint32))
    assert not np.array_equal(out1[W // 2:], out2[W // 2:])
    # and the filter did mix within a side: the left half is smoother than its input
    assert out1[:W // 2].std() < 0.7 * C[:W // 2].std()


def test_constant_frame_is_a_fixed_point_up_to_rounding():
    """Equal colours, normals and depth: every weight is h and the normalised sum returns the colour."""
    W, H = 13, 9
    C = np.full((W, H, 3), 0.75, F32)
    F = np.zeros((W, H, 8), F32)
    F[..., 0:3] = 0.5
    F[..., 5] = 1.0
    F[..., 6] = 4.0
    F[..., 7] = 1.0
    out = R.atrous(C, F, 5)
    assert np.max(np.abs(out - C)) <= 4 * np.spacing(F32(0.75))


def test_non_finite_pixels_are_set_aside():
    C, F = _frame(12, 10, 6)
    C[3, 4, 1] = np.nan
    C[8, 2, 0] = np.inf
    out = R.atrous(C, F, 3)
    assert np.array_equal(out[3, 4].view(np.uint32), C[3, 4].view(np.uint32))
    assert np.array_equal(out[8, 2].view(np.uint32), C[8, 2].view(np.uint32))
    mask = np.ones((12, 10), bool)
    mask[3, 4] = mask[8, 2] = False
    assert np.isfinite(out[mask]).all()


def test_non_finite_features_are_set_aside_too():
    """A NaN depth or an inf normal would make weights NaN: the pixel is returned unchanged, is no
    tap, and its neighbours (whose depth gradient reaches it) stay finite."""
    C, F = _frame(14, 12, 7)
    F[..., 3:6] = (0.0, 0.0, 1.0)   # one surface: every live tap has weight
    F[5, 5, 6] = np.nan
    F[9, 3, 3] = np.inf
    F[2, 8, 0] = -np.inf
    out = R.atrous(C, F, 4)
    mask = np.ones((14, 12), bool)
    for x, y in ((5, 5), (9, 3), (2, 8)):
        assert np.array_equal(out[x, y].view(np.uint32), C[x, y].view(np.uint32))
        mask[x, y] = False
    assert np.isfinite(out[mask]).all()
    assert np.any(out[4, 5] != C[4, 5]) and np.any(out[5, 6] != C[5, 6])   # the neighbours are still filtered

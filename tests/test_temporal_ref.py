"""The NumPy restatement of the temporal accumulation (tests/temporal_ref.py) against what it must mean,
without a GPU: a static sequence is a running mean, the reprojection agrees with a float64 projection,
every consistency test rejects exactly its pixels, and a pixel that is not finite stays out of the history.
tests/test_gpu_temporal.py then pins the kernel to this restatement bit for bit."""
import numpy as np
import pytest

import temporal_cases as TC
import temporal_ref as T

F32 = np.float32
W, H = 48, 40
P = T.DEFAULTS


def _moved():
    """A full plane seen from two cameras (translation plus rotation), every previous pixel with history."""
    _, cam = TC.camera((0.3, 0.2, 4.0), resolution=(W, H))
    _, pcam = TC.camera((0.1, -0.1, 3.2), looking_at=(0.15, 0.05, 0.0), up=(0.05, 1.0, 0.0), resolution=(W, H))
    rng = np.random.default_rng(7)
    F, G = TC.plane_features(cam, W, H), TC.plane_features(pcam, W, H)
    assert F[..., 7].all() and G[..., 7].all()
    C = rng.random((W, H, 3), dtype=F32) * F[..., 0:3]
    return C, F, cam, TC.random_state(rng, W, H), G, pcam


def _expected_valid(F, cam, pcam, prev_ok, cur_ok):
    """Float64 reading of steps 3 to 6: (valid, sure).  `prev_ok` marks the previous pixels a tap may use,
    `cur_ok` this frame's pixels that may reproject at all; `sure` is False where the accepted weight lies
    within 1e-3 of w_min or a tap index depends on the last bits of px, py."""
    px, py, c = TC.project64(F, cam, pcam)
    in_range = (c < 0) & (px > -1) & (px < W) & (py > -1) & (py < H)
    x0, y0 = np.floor(np.where(in_range, px, 0)), np.floor(np.where(in_range, py, 0))
    fx, fy = px - x0, py - y0
    sw = np.zeros((W, H))
    for jx, wx in ((0, 1 - fx), (1, fx)):
        for jy, wy in ((0, 1 - fy), (1, fy)):
            qx, qy = (x0 + jx).astype(int), (y0 + jy).astype(int)
            inside = in_range & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ok = inside & prev_ok[np.where(inside, qx, 0), np.where(inside, qy, 0)]
            sw += np.where(ok, wx * wy, 0.0)
    near_int = (np.abs(px - np.round(px)) < 1e-3) | (np.abs(py - np.round(py)) < 1e-3)
    sure = (np.abs(sw - P["w_min"]) > 1e-3) & ~(in_range & near_int)
    return cur_ok & (sw >= P["w_min"]), sure


@pytest.mark.parametrize("n", [2, 5, 8])
def test_a_static_sequence_is_a_running_mean(n):
    rng = np.random.default_rng(n)
    _, cam = TC.camera((0.3, 0.2, 4.0), resolution=(W, H))
    F = TC.plane_features(cam, W, H)
    F[5:9, 3:11, :] = 0                                   # some misses: they never gather history
    F[20:24, 20:24, 0] = 1e-4                             # albedo below the floor: demodulated by eps_a
    hit = F[..., 7] > 0
    frames = [(rng.random((W, H, 3), dtype=F32) * F32(3.0)) for _ in range(n)]
    prev = None
    for C in frames:
        state, color, var = T.accumulate(C, F, cam, prev, **{**P, "alpha": 0.0, "alpha_m": 0.0})
        prev = (state, F, cam)
    a = np.maximum(F[..., 0:3].astype(np.float64), np.float64(F32(P["eps_a"])))
    I = np.stack([np.where(hit[..., None], C.astype(np.float64) / a, C) for C in frames])
    bound = n * 4 * 2.0 ** -24 * np.abs(I).max()
    assert np.abs(state[hit, 0:3] - I.mean(0)[hit]).max() <= bound
    assert (state[hit, 3] == n).all()
    assert (state[~hit, 3] == 1).all() and np.array_equal(state[~hit, 0:3], frames[-1][~hit])
    assert np.array_equal(color[~hit], frames[-1][~hit])
    # the variance plane: the marker below min_history frames, a finite value >= 0 from it on
    known = np.isfinite(var)
    assert not known[~hit].any()
    assert known[hit].all() == (n >= P["min_history"]) and known[hit].any() == (n >= P["min_history"])
    assert (var[known] >= 0).all()
    assert (var[~known].view(np.uint32) == 0x7fc00000).all()


def test_b_reprojection_agrees_with_float64():
    C, F, cam, S, G, pcam = _moved()
    state, _, _, d = T.accumulate(C, F, cam, (S, G, pcam), diagnostics=True, **P)
    px, py, c = TC.project64(F, cam, pcam)
    assert (c < 0).all()
    assert np.abs(d["px"] - px).max() < 1e-3 and np.abs(d["py"] - py).max() < 1e-3
    inner = (px >= 1) & (px <= W - 2) & (py >= 1) & (py <= H - 2)
    assert inner.sum() > W * H // 3 and (~inner).sum() > W    # both kinds of pixel exist
    assert d["valid"][inner].all()
    assert (state[inner, 3] > 1).all()
    # and the cameras differ by more than a pixel almost everywhere: the test is not the static case
    x = np.arange(W)[:, None]
    assert np.median(np.abs(px - x)) > 1


def test_c_outside_the_frame():
    C, F, cam, S, G, pcam = _moved()
    _, _, _, d = T.accumulate(C, F, cam, (S, G, pcam), diagnostics=True, **P)
    all_ok = np.ones((W, H), bool)
    want, sure = _expected_valid(F, cam, pcam, all_ok, all_ok)
    assert np.array_equal(d["valid"][sure], want[sure])
    assert (~want & sure).sum() > 20 and sure.mean() > 0.9


_BLOCK = (slice(10, 30), slice(8, 25))


def _cur(change):
    def build():
        C, F, cam, S, G, pcam = _moved()
        change(F)
        cur_ok = np.ones((W, H), bool)
        cur_ok[_BLOCK] = False
        return C, F, cam, S, G, pcam, np.ones((W, H), bool), cur_ok
    return build


def _prev(change):
    def build():
        C, F, cam, S, G, pcam = _moved()
        change(S, G)
        prev_ok = np.ones((W, H), bool)
        prev_ok[_BLOCK] = False
        return C, F, cam, S, G, pcam, prev_ok, np.ones((W, H), bool)
    return build


def _set(index, value):
    def change(F):
        F[_BLOCK + (index,)] = value
    return change


def _normal(F):
    F[_BLOCK + (slice(3, 6),)] = np.array([0.0, 0.5, 0.866], F32)   # dot 0.866 < 0.9


def _depth(F):
    F[_BLOCK + (6,)] *= F32(1.04)


def _prev_depth(S, G):
    G[_BLOCK + (6,)] *= F32(1.04)


def _prev_miss(S, G):
    G[_BLOCK + (7,)] = 0


def _prev_empty(S, G):
    S[_BLOCK + (3,)] = 0


REJECTIONS = {
    "normal": _cur(_normal),
    "albedo": _cur(_set(1, F32(0.5 + 0.06))),
    "previous_depth": _prev(_prev_depth),
    "previous_miss": _prev(_prev_miss),
    "previous_h0": _prev(_prev_empty),
}


@pytest.mark.parametrize("name", sorted(REJECTIONS))
def test_c_each_rejection_resets_exactly_its_pixels(name):
    C, F, cam, S, G, pcam, prev_ok, cur_ok = REJECTIONS[name]()
    state, _, var, d = T.accumulate(C, F, cam, (S, G, pcam), diagnostics=True, **P)
    want, sure = _expected_valid(F, cam, pcam, prev_ok, cur_ok)
    base, _ = _expected_valid(F, cam, pcam, np.ones((W, H), bool), np.ones((W, H), bool))
    assert np.array_equal(d["valid"][sure], want[sure])
    assert ((base & ~want) & sure).sum() > 50            # the rejection did reset pixels the base case keeps
    reset = ~d["valid"]
    assert (state[reset, 3] == 1).all() and (var[reset].view(np.uint32) == 0x7fc00000).all()
    hit = F[..., 7] > 0
    a = np.fmax(F[..., 0:3], F32(P["eps_a"]))
    assert np.array_equal(state[reset & hit, 0:3], (C / a)[reset & hit])


def test_c_this_frames_depth_moves_the_point():
    """A depth 4 % off puts the point elsewhere; where that still lands in the frame the previous surface
    is 4 % nearer than the point, which tau_z = 0.02 rejects."""
    C, F, cam, S, G, pcam = _moved()
    _depth(F)
    _, _, _, d = T.accumulate(C, F, cam, (S, G, pcam), diagnostics=True, **P)
    assert not d["valid"][_BLOCK].any()
    outside = np.ones((W, H), bool)
    outside[_BLOCK] = False
    _, _, _, d0 = T.accumulate(C, _moved()[1], cam, (S, G, pcam), diagnostics=True, **P)
    assert np.array_equal(d["valid"][outside], d0["valid"][outside])


def test_c_behind_the_previous_camera():
    C, F, cam, S, G, _ = _moved()
    _, away = TC.camera((0.0, 0.0, 3.0), looking_at=(0.0, 0.0, 9.0), resolution=(W, H))
    # the previous camera looks away from the plane: G stays a full, consistent frame, so only c >= 0 rejects
    state, _, _, d = T.accumulate(C, F, cam, (S, G, away), diagnostics=True, **P)
    _, _, c = TC.project64(F, cam, away)
    assert (c > 0).all()
    assert not d["valid"].any() and not d["in_range"].any()
    assert (state[..., 3] == 1).all()
    # mirrored through the eye the same points would project into the frame: the sign of c is what rejects
    px, py, _ = TC.project64(F, cam, away)
    assert ((px > 0) & (px < W - 1) & (py > 0) & (py < H - 1)).any()


def test_c_a_miss_and_the_first_frame_have_no_history():
    C, F, cam, S, G, pcam = _moved()
    F[_BLOCK + (slice(0, 8),)] = 0
    state, color, var, d = T.accumulate(C, F, cam, (S, G, pcam), diagnostics=True, **P)
    assert not d["valid"][_BLOCK].any() and (state[_BLOCK + (3,)] == 1).all()
    assert np.array_equal(color[_BLOCK], C[_BLOCK])
    first, color1, var1 = T.accumulate(C, F, cam, None, **P)
    assert (first[..., 3] == 1).all() and (var1.view(np.uint32) == 0x7fc00000).all()
    assert np.array_equal(first[..., 4] * first[..., 4], first[..., 5])


def test_d_a_bad_pixel_neither_receives_nor_donates():
    C, F, cam, S, G, pcam = _moved()
    bad = np.zeros((W, H), bool)
    bad[12, 9] = bad[30, 30] = bad[31, 30] = True
    C1 = C.copy()
    C1[12, 9, 1] = np.nan
    C1[30, 30, 0] = np.inf
    F1 = F.copy()
    F1[31, 30, 6] = np.nan
    # receives nothing: whatever the previous frame holds, its state is empty and its colour passes through
    state, color, var = T.accumulate(C1, F1, cam, (S, G, pcam), **P)
    assert not state[bad].any()
    assert np.array_equal(color[bad].view(np.uint32), C1[bad].view(np.uint32))
    assert (var[bad].view(np.uint32) == 0x7fc00000).all()
    clean = T.accumulate(C, F, cam, (S, G, pcam), **P)[0]
    assert np.array_equal(state[~bad].view(np.uint32), clean[~bad].view(np.uint32))
    # donates nothing: seen from the next camera, its taps count as little as a pixel without history
    nxt_cam = pcam
    F2 = TC.plane_features(nxt_cam, W, H)
    C2 = np.random.default_rng(3).random((W, H, 3), dtype=F32)
    s2, c2, v2, d = T.accumulate(C2, F2, nxt_cam, (state, F1, cam), diagnostics=True, **P)
    ok_prev = ~bad
    want, sure = _expected_valid(F2, nxt_cam, cam, ok_prev, np.ones((W, H), bool))
    assert np.array_equal(d["valid"][sure], want[sure])
    assert np.isfinite(s2[..., 0:6]).all() and np.isfinite(c2).all()
    poisoned = state.copy()
    poisoned[bad, 0:3] = 1e30                              # h stays 0: values of an empty history are never read
    s3 = T.accumulate(C2, F2, nxt_cam, (poisoned, F1, cam), **P)[0]
    assert np.array_equal(s2.view(np.uint32), s3.view(np.uint32))


def test_mixed_select():
    live = np.array([[True, True, True, True, True, False]])
    est = np.array([[1, 2, 3, 4, 5, 0]], F32)
    t = np.array([[0.5, np.nan, np.inf, -1.0, -0.0, 9.0]], F32)
    got = T.mixed(t, est, live)
    assert np.array_equal(got.view(np.uint32), np.array([[0.5, 2, 3, 4, -0.0, 0]], F32).view(np.uint32))

"""Adaptive sampling on the GPU: prt_adaptive_update and its device form against the NumPy restatement
(tests/adaptive_ref.py) bit for bit, and AdaptiveAccumulator end to end against the existing path: uniform
batches from render_tiles_accumulate pushed through the restatement and the policy.

End-to-end figures (Cornell 32 x 32, tile 8, depth 4, 4 spp per batch, 8 batches, seed 3), as
test_the_sampler_reproduces_the_reference_path prints them on the MI355X: target 0.8516472578048706 (bits
0x3f5a058e, the 8th smallest after the 4th batch: the quantile and the batch index the issue names, unchanged),
batches per tile [4, 4, 7, 3, 3, 6, 8, 7, 2, 3, 2, 4, 8, 8, 8, 8] from the reference path and from the sampler."""
import os

import numpy as np
import pytest

import adaptive_ref as A
import moments_ref as M
from denoise_cases import bits
from moments_cases import BOUND, N_SAMPLES, PAR, frames

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS_R, TARGET = 1e-3, 0.2
SENTINEL = np.uint32(0x7FC12345)   # a NaN with a payload: arithmetic on it would change the bits
# frame, tile: one full tile (one wave); three of four tiles partial; tw != th; several chunks per tile; a tile
# wider than the frame
SHAPES = [(8, 8, 8, 8), (13, 9, 8, 8), (37, 19, 16, 4), (70, 130, 32, 32), (70, 130, 64, 64)]
K = 3


def _lists(n, rng):
    """The full list, a shuffled strict subset, a single tile and the empty list."""
    full = np.arange(n, dtype=np.int32)
    if n == 1:
        return dict(full=full, empty=full[:0])
    sub = rng.permutation(n)[: max(1, n - 1 - n // 3)].astype(np.int32)
    return dict(full=full, subset=sub, single=np.array([n - 1], np.int32), empty=full[:0])


@pytest.fixture(scope="module")
def restated():
    """Per shape: the K frames of sums, the features and, per list, the restatement's (sum, state, records)
    after each of the K batches.  Planes start as the sentinel outside the listed tiles and empty inside."""
    out = {}
    for W, H, tw, th in SHAPES:
        S, F = frames(W, H, K, 700 + 10 * W + tw)
        n = A.n_tiles(tw, th, W, H)
        per_list = {}
        for name, ids in _lists(n, np.random.default_rng(W + tw)).items():
            s, st = _start(W, H, tw, th, ids)
            steps = []
            for k in range(K):
                s, st, rec = A.update(s, st, A.pack(S[k], ids, tw, th), ids, tw, th, F, N_SAMPLES, PAR["eps_a"], EPS_R,
                                      TARGET)
                steps.append((s, st, rec))
            per_list[name] = (ids, steps)
        out[(W, H, tw, th)] = (S, F, per_list)
    return out


def _start(W, H, tw, th, ids):
    s = np.zeros((W, H, 3), F32)
    st = np.zeros((W, H, 4), F32)
    s.view(np.uint32)[...] = SENTINEL
    st.view(np.uint32)[...] = SENTINEL
    for tid in ids:
        x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
        s[x0:x0 + w, y0:y0 + h] = 0
        st[x0:x0 + w, y0:y0 + h] = 0
    return s, st


def _listed(W, H, tw, th, ids):
    m = np.zeros((W, H), bool)
    for tid in ids:
        x0, y0, w, h = A.tile_rect(tid, tw, th, W, H)
        m[x0:x0 + w, y0:y0 + h] = True
    return m


@pytest.mark.parametrize("W,H,tw,th", SHAPES)
def test_update_equals_the_restatement_bit_for_bit(restated, W, H, tw, th):
    from pyrenderer_amd.adaptive import adaptive_update
    from pyrenderer_amd.denoise import moments_add, moments_state
    S, F, per_list = restated[(W, H, tw, th)]
    for name, (ids, steps) in per_list.items():
        s, st = _start(W, H, tw, th, ids)
        listed = _listed(W, H, tw, th, ids)
        for k in range(K):
            rec = adaptive_update(s, st, A.pack(S[k], ids, tw, th), ids, tw, th, F, N_SAMPLES, target=TARGET, eps_r=EPS_R,
                                  eps_a=PAR["eps_a"])
            want_s, want_st, want_rec = steps[k]
            assert rec.shape == (len(ids), 4) and np.array_equal(rec, want_rec), (name, k, rec, want_rec)
            diff = np.argwhere(np.any(bits(st) != bits(want_st), axis=-1))
            assert len(diff) == 0, (name, k, len(diff), diff[:5], st[tuple(diff[0])], want_st[tuple(diff[0])])
            diff = np.argwhere(np.any(bits(s) != bits(want_s), axis=-1))
            assert len(diff) == 0, (name, k, len(diff), diff[:5])
            # pixels of tiles that are not listed keep their sentinel bits
            assert (bits(s)[~listed] == SENTINEL).all() and (bits(st)[~listed] == SENTINEL).all(), (name, k)
        if name == "full":
            # the full list is prt_moments_add, and what the inputs exercise shows in the records
            want = moments_add(moments_state(W, H), S, N_SAMPLES, F, eps_a=PAR["eps_a"])
            assert np.array_equal(bits(st), bits(want))
            assert np.array_equal(bits(st), bits(M.moments_add(np.zeros((W, H, 4), F32), S, N_SAMPLES, F, PAR["eps_a"])))
            assert np.isfinite(st).all() and st[W - 1, H - 1, 2] >= BOUND * BOUND
            assert int(rec[:, 0].sum()) == W * H and not rec[:, 3].any()
            first = steps[0][2]
            assert np.array_equal(first[:, 0], first[:, 1]) and first[:, 3].sum() == W * H   # one batch: all young
            assert (st[..., 0] == K).sum() == W * H - 2 and (st[..., 0] == K - 1).sum() == 2   # the NaN and the inf
            assert (rec[:, 1] > 0).any() and (rec[:, 1] < rec[:, 0]).any()   # the target splits the pixels
            assert (F[..., 7] == 0).any() and (F[..., 0] < PAR["eps_a"]).any()


def test_device_form_on_a_side_stream_in_halves_and_inside_its_arrays(restated):
    """Two calls over disjoint halves of a list equal one call; guard words around every array stay as they were."""
    import torch
    from pyrenderer_amd.adaptive import adaptive_update_device
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    GUARD = 64   # floats on either side; 256 bytes keep the state 16-byte aligned
    for shape in [(70, 130, 32, 32), (13, 9, 8, 8), (37, 19, 16, 4)]:
        W, H, tw, th = shape
        S, F, per_list = restated[shape]
        ids, steps = per_list["subset"] if "subset" in per_list else per_list["full"]
        half = len(ids) // 2
        s0, st0 = _start(W, H, tw, th, ids)

        def padded(a, value):
            flat = np.full(a.size + 2 * GUARD, value, a.dtype)
            flat[GUARD:GUARD + a.size] = a.reshape(-1)
            return torch.from_numpy(flat).to(dev)

        d_s, d_st = padded(s0, 7.0), padded(st0, 7.0)
        d_f = padded(F, 7.0)
        d_rec = torch.full((len(ids) * 4 + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        assert (d_st.data_ptr() + GUARD * 4) % 16 == 0
        for k in range(K):
            batch = A.pack(S[k], ids, tw, th)
            d_b = padded(batch, 7.0)
            stream.wait_stream(torch.cuda.current_stream(dev))
            for lo, hi in ((0, half), (half, len(ids))):
                adaptive_update_device(d_b.data_ptr() + (GUARD + lo * tw * th * 3) * 4, ids[lo:hi], tw, th, W, H,
                                       d_f.data_ptr() + GUARD * 4, N_SAMPLES, d_s.data_ptr() + GUARD * 4,
                                       d_st.data_ptr() + GUARD * 4, d_rec.data_ptr() + (GUARD + lo * 4) * 4,
                                       target=TARGET, eps_r=EPS_R, eps_a=PAR["eps_a"], stream_ptr=stream.cuda_stream)
            stream.synchronize()
            want_s, want_st, want_rec = steps[k]
            got_s, got_st, got_rec = d_s.cpu().numpy(), d_st.cpu().numpy(), d_rec.cpu().numpy().view(np.uint32)
            assert np.array_equal(got_rec[GUARD:-GUARD].reshape(-1, 4), want_rec), (shape, k)
            assert np.array_equal(bits(got_s[GUARD:-GUARD]), bits(want_s).reshape(-1)), (shape, k)
            assert np.array_equal(bits(got_st[GUARD:-GUARD]), bits(want_st).reshape(-1)), (shape, k)
            for g in (got_s, got_st, d_f.cpu().numpy(), d_b.cpu().numpy()):
                assert (g[:GUARD] == 7.0).all() and (g[-GUARD:] == 7.0).all(), (shape, k)
            assert (got_rec[:GUARD] == 0x5A5A5A5A).all() and (got_rec[-GUARD:] == 0x5A5A5A5A).all(), (shape, k)
            assert np.array_equal(bits(d_f.cpu().numpy()[GUARD:-GUARD]), bits(F).reshape(-1))


# -------------------------------------------------------------- end to end ----

E2E = dict(depth=4, seed=3, resolution=(32, 32), tile=8)
BATCH_SPP, MAX_BATCHES, QUANTILE, AT_BATCH = 4, 8, 8, 4


@pytest.fixture(scope="module")
def reference_path(cornell):
    """The existing path: eight uniform batches of all 16 tiles from render_tiles_accumulate onto zeros, and the
    one-sample features; then the restatement and the policy in NumPy for a target."""
    from pyrenderer_amd.core.tracing import _Frame, build_world
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    f = _Frame.of(scene, cam, world=world, **E2E)
    W, H, t = f.W, f.H, f.tile
    batches = [f.unpack(f.add_samples(b * BATCH_SPP, BATCH_SPP)) for b in range(MAX_BATCHES)]
    feat = f.features()
    n = A.n_tiles(t, t, W, H)

    def run(target, min_batches=2, tolerate=0.0):
        """(batches per tile, sums, state, every round's records by tile id) of the reference path."""
        from pyrenderer_amd.adaptive import EPS_R as DEFAULT_EPS_R, still_active
        from pyrenderer_amd.denoise import EPS_A
        active, per_tile = np.ones(n, bool), np.zeros(n, np.int32)
        s, st = np.zeros((W, H, 3), F32), np.zeros((W, H, 4), F32)
        rounds = []
        for b in range(1, MAX_BATCHES + 1):
            ids = np.nonzero(active)[0]
            if len(ids) == 0:
                break
            s, st, rec = A.update(s, st, A.pack(batches[b - 1], ids, t, t), ids, t, t, feat, BATCH_SPP, EPS_A,
                                  DEFAULT_EPS_R, target)
            by_id = np.zeros((n, 4), np.uint32)
            by_id[ids] = rec
            rounds.append(by_id)
            per_tile[ids] = b
            active[ids] = still_active(rec, b, min_batches, tolerate)
        return per_tile, s, st, rounds

    return scene, cam, world, batches, feat, run


def test_the_sampler_reproduces_the_reference_path(reference_path):
    """The target is the 8th smallest of the 16 tiles' record word [2] after the 4th uniform batch, as that exact
    f32: about half of the tiles are below it then, and some of those were already below it earlier."""
    from pyrenderer_amd.adaptive import AdaptiveAccumulator
    from pyrenderer_amd.core.tracing import Accumulator
    scene, cam, world, batches, feat, run = reference_path
    uniform = run(0.0)
    assert (uniform[0] == MAX_BATCHES).all()
    word2 = np.sort(uniform[3][AT_BATCH - 1][:, 2])
    target = float(word2[QUANTILE - 1:QUANTILE].view(F32)[0])
    want_map, want_s, want_st, want_rounds = run(target)
    print(f"adaptive e2e: target {target!r} (bits {int(word2[QUANTILE - 1]):#x}); reference batches per tile "
          f"{want_map.tolist()}")
    # the reference's own map is mixed: a tile that stops before batch 8 and a tile that runs past batch 4
    assert len(set(want_map.tolist())) >= 2 and want_map.min() < MAX_BATCHES and want_map.max() > AT_BATCH, want_map

    acc = AdaptiveAccumulator(scene, cam, batch_spp=BATCH_SPP, target=target, world=world, **E2E).run(MAX_BATCHES)
    print(f"adaptive e2e: sampler batches per tile {acc.batches_per_tile.tolist()}")
    assert np.array_equal(acc.batches_per_tile, want_map)
    assert np.array_equal(bits(acc.sums()), bits(want_s)) and np.array_equal(bits(acc.moments()), bits(want_st))
    assert np.array_equal(acc.samples(), np.repeat(np.repeat(want_map.reshape(4, 4).T, 8, 0), 8, 1) * BATCH_SPP)
    last = np.zeros_like(want_rounds[0])
    for r in want_rounds:
        last = np.where(r[:, :1] > 0, r, last)
    assert np.array_equal(acc.records(), last)
    assert np.array_equal(bits(acc.features()), bits(feat))
    assert np.array_equal(bits(acc.noise_map()), bits(np.sqrt(want_st[..., 3])))
    assert np.array_equal(bits(acc.mean()), bits(want_s / acc.samples().astype(F32)[..., None]))
    # tile for tile the snapshot Accumulator(moments=True) holds after k_t equal add()s
    plain = Accumulator(scene, cam, moments=True, world=world, **E2E)
    for k in range(1, MAX_BATCHES + 1):
        plain.add(BATCH_SPP)
        for tid in np.nonzero(want_map == k)[0]:
            x0, y0, w, h = A.tile_rect(tid, 8, 8, 32, 32)
            r = (slice(x0, x0 + w), slice(y0, y0 + h))
            assert np.array_equal(bits(acc.sums()[r]), bits(plain.sums()[r])), (k, tid)
            assert np.array_equal(bits(acc.moments()[r]), bits(plain.moments_state[r])), (k, tid)


def test_target_zero_is_uniform_and_infinity_stops_at_two(reference_path):
    from pyrenderer_amd.adaptive import AdaptiveAccumulator
    scene, cam, world, batches, feat, run = reference_path
    zero = AdaptiveAccumulator(scene, cam, batch_spp=BATCH_SPP, target=0.0, world=world, **E2E).run(MAX_BATCHES)
    assert (zero.batches_per_tile == MAX_BATCHES).all() and zero.active.all()
    total = np.zeros_like(batches[0])
    for b in batches:
        total = total + b
    assert np.array_equal(bits(zero.sums()), bits(total))
    assert np.array_equal(bits(zero.moments()), bits(M.moments_add(np.zeros((32, 32, 4), F32), np.stack(batches),
                                                                    BATCH_SPP, feat)))
    inf = AdaptiveAccumulator(scene, cam, batch_spp=BATCH_SPP, target=np.inf, world=world, **E2E).run(MAX_BATCHES)
    assert (inf.batches_per_tile == 2).all() and not inf.active.any() and inf.batches == 2
    assert np.array_equal(bits(inf.sums()), bits(batches[0] + batches[1]))
    three = AdaptiveAccumulator(scene, cam, batch_spp=BATCH_SPP, target=np.inf, min_batches=3, world=world, **E2E)
    assert three.step() == 16 and three.step() == 16 and three.step() == 0 and three.step() == 0
    assert (three.batches_per_tile == 3).all()


def test_render_adaptive_and_the_command_line(reference_path, tmp_path):
    from pyrenderer_amd.core.tracing import render_adaptive
    from pyrenderer_amd.main import main
    scene, cam, world, batches, feat, run = reference_path
    target = 0.1
    want_map, want_s, _, _ = run(target)
    img, samples = render_adaptive(scene, cam, batch_spp=BATCH_SPP, max_batches=MAX_BATCHES, target=target, world=world,
                                   return_samples=True, **E2E)
    assert samples.shape == (32, 32) and samples.dtype == np.int32
    assert np.array_equal(bits(img), bits(want_s / samples.astype(F32)[..., None]))
    den = render_adaptive(scene, cam, batch_spp=BATCH_SPP, max_batches=MAX_BATCHES, target=target, world=world,
                          denoise="variance", **E2E)
    assert den.shape == (32, 32, 3) and np.isfinite(den).all() and not np.array_equal(den, img)
    fixed = render_adaptive(scene, cam, batch_spp=BATCH_SPP, max_batches=MAX_BATCHES, target=target, world=world,
                            denoise=True, **E2E)
    assert np.isfinite(fixed).all() and not np.array_equal(fixed, den)
    # the command line renders 64-pixel tiles: one tile at 32 x 32, so its map is one number
    aov = str(tmp_path / "aov")
    out = main(["--resolution", "32", "32", "--depth", "4", "--seed", "3", "--adaptive", "inf", "--batch-spp", "4",
                "--max-samples", "32", "--min-batches", "3", "--aov", aov, "--out", str(tmp_path / "a.png")])
    got = np.load(os.path.join(aov, "samples.npy"))
    assert sorted(os.listdir(aov)) == ["albedo.png", "depth.npy", "normal.png", "samples.npy"]
    assert got.shape == (32, 32) and got.dtype == np.int32 and (got == 12).all()
    assert np.array_equal(bits(out), bits(((batches[0] + batches[1]) + batches[2]) / F32(12)))

"""The orchestration above libprt, without a GPU: which renders, feature passes and filters render(),
render_batches(), Accumulator and the command line ask for, in which order, and with which arguments.

The device is a recording fake behind the `world=` argument; the four functions of pyrenderer_amd.denoise
that reach the GPU are recording fakes too.  Cornell's camera at 72 x 40 with 64-pixel tiles gives two
tiles, ragged in x and in y."""
import types

import numpy as np
import pytest

from conftest import CORNELL_JSON

F32 = np.float32
W, H, TILE, DEPTH, SEED = 72, 40, 64, 4, 3
N_TILES = 2
CLI = ["--resolution", str(W), str(H), "--depth", str(DEPTH), "--seed", str(SEED), "--samples", "8", "--out", ""]
VARIANCE = ["--denoise", "--denoise-mode", "variance"]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _radiance(ids, tw, th, sample, seed):
    """(n_tiles * tw * th, 3) float32 in [0.1, 1.1): a fixed function of (tile id, slot, sample, seed)."""
    tid = np.asarray(ids, np.int64)[:, None, None]
    slot = np.arange(tw * th, dtype=np.int64)[None, :, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    h = (tid * 7919 + slot * 31 + c * 7 + sample * 40503 + seed * 97 + 1) * 2654435761 % 65521
    return (h.astype(F32) / F32(65521) + F32(0.1)).reshape(-1, 3)


class FakeDeviceScene:
    def __init__(self, log):
        self.log = log

    def render_tiles(self, cam, W, H, tw, th, tile_ids, spp, depth, seed=0, flags=0):
        self.log.append(("render_tiles", 0, int(spp), len(tile_ids)))
        out = np.zeros((len(tile_ids) * tw * th, 3), F32)
        for s in range(spp):
            out += _radiance(tile_ids, tw, th, s, seed)
        return out, np.zeros(4, np.uint64)

    def render_tiles_accumulate(self, cam, W, H, tw, th, tile_ids, first_sample, spp, depth, sums, seed=0, flags=0):
        self.log.append(("accumulate", int(first_sample), int(spp), len(tile_ids)))
        assert sums.shape == (len(tile_ids) * tw * th, 3) and sums.dtype == F32
        for s in range(first_sample, first_sample + spp):
            sums += _radiance(tile_ids, tw, th, s, seed)
        return sums


class FakeWorld:
    def __init__(self, log):
        self.flat = types.SimpleNamespace(tri_v=np.arange(9, dtype=F32))
        self.scenes = {}
        self.log = log

    def device_scene(self, device=0):
        return self.scenes.setdefault(device, FakeDeviceScene(self.log))


@pytest.fixture(scope="module")
def camera():
    from pyrenderer_amd.io_utils.read_tungsten import read_file
    return read_file(CORNELL_JSON)[1]


@pytest.fixture
def rig(camera, monkeypatch):
    """The fake world, the shared call log and the patched denoise module.  log entries: the fake device's
    (name, first_sample, spp, n_tiles); ("features", samples, seed, tile); ("moments", n_frames, n_samples);
    ("denoise" | "denoise_variance", mean, feat, keyword arguments)."""
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd import main as M
    from pyrenderer_amd.core import tracing as T
    log = []
    world = FakeWorld(log)

    def features_packed(ds, cam_packed, w, h, *, samples=1, seed=0, tile=64, **kw):
        assert isinstance(ds, FakeDeviceScene) and (int(w), int(h)) == (W, H)
        log.append(("features", samples, seed, tile))
        f = np.zeros((W, H, 8), F32)
        f[...] = (np.arange(W, dtype=F32)[:, None, None] + F32(2) * np.arange(H, dtype=F32)[None, :, None]
                  + np.arange(8, dtype=F32)[None, None, :] + F32(seed))
        return f

    def moments_add(state, sums_frames, n_samples, feat, *, eps_a=D.EPS_A, device=0):
        frames = np.asarray(sums_frames, F32)
        frames = frames[None] if frames.ndim == 3 else frames
        assert frames.shape[1:] == (W, H, 3) and state.shape == (W, H, 4) and feat.shape == (W, H, 8)
        log.append(("moments", frames.shape[0], n_samples))
        for fr in frames:
            state[..., 0] += F32(1)
            state[..., 3] += fr.sum(axis=-1) / F32(n_samples) * F32(0.125)
        return state

    def denoise(mean, feat, **kw):
        log.append(("denoise", np.array(mean), feat, kw))
        return np.asarray(mean, F32) * F32(0.5) + F32(1)

    def denoise_variance(mean, feat, *, return_variance=False, variance=None, **kw):
        log.append(("denoise_variance", np.array(mean), feat, dict(kw, variance=variance)))
        var = np.full((W, H), F32(2)) if variance is None else np.asarray(variance, F32)
        out = np.asarray(mean, F32) * F32(0.25) + var[..., None]
        return (out, var) if return_variance else out

    for fn in (features_packed, moments_add, denoise, denoise_variance):
        monkeypatch.setattr(D, fn.__name__, fn)
    monkeypatch.setattr(T, "build_world", lambda scene, devices=(0,): world)
    monkeypatch.setattr(M, "build_world", lambda scene, devices=(0,): world, raising=False)
    monkeypatch.setattr(M, "read_file", lambda path: ("the scene", camera))
    return types.SimpleNamespace(world=world, log=log, kw=dict(depth=DEPTH, seed=SEED, resolution=(W, H), world=world))


def _frame_of(slots):
    """Slot rows (tile-major, then row ly, then column lx) of tiles 0 and 1 as the (W, H, C) frame, by index."""
    x, y = np.arange(W)[:, None], np.arange(H)[None, :]
    return slots[(x // TILE) * TILE * TILE + (y % TILE) * TILE + x % TILE]


def _device_calls(log):
    return [e for e in log if e[0] in ("render_tiles", "accumulate")]


def _count(log, name):
    return sum(e[0] == name for e in log)


def _filters(log):
    return [e for e in log if e[0] in ("denoise", "denoise_variance")]


BATCHED = [("accumulate", 0, 2, N_TILES), ("accumulate", 2, 2, N_TILES), ("accumulate", 4, 2, N_TILES),
           ("accumulate", 6, 2, N_TILES)]
# per mode: render()'s keywords, the command line's switches, the device calls, the filter
MODES = {
    "plain": (dict(), [], [("render_tiles", 0, 8, N_TILES)], None),
    "fixed": (dict(denoise=True), ["--denoise"], [("render_tiles", 0, 8, N_TILES)], "denoise"),
    "variance": (dict(denoise="variance"), VARIANCE, [("render_tiles", 0, 8, N_TILES)], "denoise_variance"),
    "moments": (dict(denoise="variance", variance_batches=4), VARIANCE + ["--variance-batches", "4"], BATCHED,
                "denoise_variance"),
}


def _render(rig, camera, mode):
    """render() in `mode`: (image, the calls it made)."""
    from pyrenderer_amd.core.tracing import render
    del rig.log[:]
    img = render("the scene", camera, spp=8, **MODES[mode][0], **rig.kw)
    return img, list(rig.log)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_render_asks_for_these_calls(rig, camera, mode):
    from pyrenderer_amd.core.tracing import render, render_batches
    _, _, device_calls, filt = MODES[mode]
    img, log = _render(rig, camera, mode)
    assert img.shape == (W, H, 3) and img.dtype == F32
    assert _device_calls(log) == device_calls
    assert _count(log, "features") == (1 if filt else 0)
    assert [e for e in log if e[0] == "features"] == ([("features", 1, SEED, TILE)] if filt else [])
    assert [e[0] for e in _filters(log)] == ([filt] if filt else [])
    if not filt:
        return
    _, mean, feat, kw = _filters(log)[0]
    if mode == "moments":
        assert [e for e in log if e[0] == "moments"] == [("moments", 4, 2)]
        sums, bfeat, state = render_batches("the scene", camera, spp=8, variance_batches=4, **rig.kw)
        assert np.array_equal(_bits(mean), _bits(sums / F32(8)))
        assert np.array_equal(_bits(kw["variance"]), _bits(state[..., 3])) and state[..., 3].any()
        assert np.array_equal(_bits(feat), _bits(bfeat))
    else:
        assert np.array_equal(_bits(mean), _bits(render("the scene", camera, spp=8, **rig.kw)))
        assert kw.get("variance") is None
    assert {k: v for k, v in kw.items() if k != "variance"} == {"device": 0}


def test_render_batches_calls_and_sums(rig, camera):
    from pyrenderer_amd.core.tracing import render_batches
    from pyrenderer_amd.device_scene import interleaved_tiles
    sums, feat, state = render_batches("the scene", camera, spp=8, variance_batches=4, **rig.kw)
    assert _device_calls(rig.log) == BATCHED and _count(rig.log, "features") == 1
    assert (state[..., 0] == 4).all() and feat.shape == (W, H, 8)
    # the batch sums, each from zero, added in batch order before the unpack
    ids = interleaved_tiles(W, H, TILE)
    total = np.zeros((N_TILES * TILE * TILE, 3), F32)
    for j in range(4):
        batch = np.zeros_like(total)
        for s in range(2 * j, 2 * j + 2):
            batch += _radiance(ids, TILE, TILE, s, SEED)
        total += batch
    assert np.array_equal(_bits(sums), _bits(_frame_of(total)))


def test_sample_order_sums_and_empty_renders(rig, camera):
    from pyrenderer_amd.core.tracing import Accumulator, render, render_sums
    from pyrenderer_amd.device_scene import interleaved_tiles
    ids = interleaved_tiles(W, H, TILE)
    want = np.zeros((N_TILES * TILE * TILE, 3), F32)
    for s in range(8):
        want += _radiance(ids, TILE, TILE, s, SEED)
    want = _frame_of(want)
    sums = render_sums("the scene", camera, spp=8, **rig.kw)
    assert np.array_equal(_bits(sums), _bits(want))
    assert np.array_equal(_bits(render("the scene", camera, spp=8, **rig.kw)), _bits(want / F32(8)))
    del rig.log[:]
    for fn in (render, render_sums):
        z = fn("the scene", camera, spp=0, **rig.kw)
        assert z.shape == (W, H, 3) and z.dtype == F32 and not z.any()
    acc = Accumulator("the scene", camera, **rig.kw)
    assert not acc.mean().any() and acc.mean().shape == (W, H, 3)
    assert rig.log == []


def test_accumulator_without_moments(rig, camera, tmp_path):
    from pyrenderer_amd.core.tracing import Accumulator, render
    acc = Accumulator("the scene", camera, **rig.kw)
    assert acc.add(3).add(5) is acc and acc.samples == 8
    assert rig.log == [("accumulate", 0, 3, N_TILES), ("accumulate", 3, 5, N_TILES)]
    plain, _ = _render(rig, camera, "plain")
    assert np.array_equal(_bits(acc.mean()), _bits(plain))
    for mode, name in (("fixed", "denoise"), ("variance", "denoise_variance")):
        del rig.log[:]
        got = acc.denoised(mode=mode, sigma_z=1.5)
        # one feature pass for the first filter; a later one may reuse it
        assert _count(rig.log, "features") <= 1 and _device_calls(rig.log) == []
        assert _count(rig.log, "features") == 1 or mode != "fixed"
        (fname, mean, _, kw), = _filters(rig.log)
        assert fname == name and np.array_equal(_bits(mean), _bits(plain))
        assert kw.get("variance") is None and kw["sigma_z"] == 1.5 and kw["device"] == 0
        want, _ = _render(rig, camera, mode)
        assert got.shape == want.shape
    assert np.array_equal(_bits(acc.denoised()), _bits(_render(rig, camera, "fixed")[0]))
    assert np.array_equal(_bits(acc.denoised(mode="variance")), _bits(_render(rig, camera, "variance")[0]))
    with pytest.raises(ValueError, match="mode"):
        acc.denoised(mode="nonsense")
    acc.save(tmp_path / "acc")
    z = np.load(tmp_path / "acc.npz")
    assert sorted(z.files) == sorted(["slots", "samples", "seed", "depth", "resolution", "tile", "flags", "camera",
                                      "scene_sha"])
    back = Accumulator.load(tmp_path / "acc", "the scene", camera, world=rig.world)
    assert back.samples == 8 and not back.moments and np.array_equal(_bits(back.sums()), _bits(acc.sums()))
    other = FakeWorld([])
    other.flat.tri_v = other.flat.tri_v + F32(1)
    with pytest.raises(ValueError, match="different scene"):
        Accumulator.load(tmp_path / "acc", "the scene", camera, world=other)


def test_accumulator_with_moments(rig, camera, tmp_path):
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import Accumulator
    acc = Accumulator("the scene", camera, moments=True, **rig.kw)
    given = np.full((W, H), F32(7))
    for batches in (1, 2, 3, 4):
        acc.add(2)
        if batches == 1:
            continue
        assert acc.batches == batches
        del rig.log[:]
        acc.denoised("variance")
        (_, mean, _, kw), = _filters(rig.log)
        assert np.array_equal(_bits(mean), _bits(acc.mean()))
        if batches < D.MIN_MOMENT_BATCHES:
            assert kw.get("variance") is None
        else:
            assert np.array_equal(_bits(kw["variance"]), _bits(acc.moments_state[..., 3])) and kw["variance"].any()
        acc.denoised("variance", variance=given)
        assert _filters(rig.log)[-1][3]["variance"] is given
        acc.denoised("fixed")
        assert _filters(rig.log)[-1][0] == "denoise" and "variance" not in _filters(rig.log)[-1][3]
        assert _count(rig.log, "features") == 0 and _device_calls(rig.log) == []   # composed once, with batch 1
    want, _ = _render(rig, camera, "moments")
    assert np.array_equal(_bits(acc.denoised("variance")), _bits(want))
    assert np.array_equal(_bits(acc.noise_map()), _bits(np.sqrt(acc.moments_state[..., 3])))
    # the whole accumulation asked for the four batches, one feature pass and one moments update per batch
    acc2 = Accumulator("the scene", camera, moments=True, **rig.kw)
    del rig.log[:]
    for _ in range(4):
        acc2.add(2)
    acc2.denoised("variance")
    assert _device_calls(rig.log) == BATCHED and _count(rig.log, "features") == 1
    assert [e for e in rig.log if e[0] == "moments"] == [("moments", 1, 2)] * 4
    assert np.array_equal(_bits(acc2.moments_state), _bits(acc.moments_state))
    acc.save(tmp_path / "m.npz")
    assert sorted(np.load(tmp_path / "m.npz").files) == sorted(
        ["slots", "samples", "seed", "depth", "resolution", "tile", "flags", "camera", "scene_sha", "moments",
         "batch_spp"])
    back = Accumulator.load(tmp_path / "m.npz", "the scene", camera, world=rig.world)
    assert back.moments and back.batch_spp == 2 and back.batches == 4
    assert np.array_equal(_bits(back.denoised("variance")), _bits(want))
    # a file whose slot sums do not cover its own resolution and tile is refused
    z = dict(np.load(tmp_path / "m.npz"))
    z["slots"] = z["slots"][:-1]
    np.savez(tmp_path / "m.npz", **z)
    with pytest.raises(ValueError, match="layout"):
        Accumulator.load(tmp_path / "m.npz", "the scene", camera, world=rig.world)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_command_line_is_render(rig, camera, mode):
    from pyrenderer_amd.main import main
    want, want_log = _render(rig, camera, mode)
    del rig.log[:]
    got = main(CLI + MODES[mode][1])
    assert np.array_equal(_bits(got), _bits(want))
    assert _device_calls(rig.log) == _device_calls(want_log)
    assert _count(rig.log, "features") == _count(want_log, "features")
    assert [e[0] for e in _filters(rig.log)] == [e[0] for e in _filters(want_log)]
    for a, b in zip(_filters(rig.log), _filters(want_log)):
        assert np.array_equal(_bits(a[1]), _bits(b[1]))


def test_progressive_command_line_is_the_accumulator(rig, camera, tmp_path):
    from pyrenderer_amd.core.tracing import Accumulator
    from pyrenderer_amd.main import main
    aov = str(tmp_path / "aov")
    got = main(CLI + VARIANCE + ["--interval", "2", "--variance-batches", "4", "--aov", aov])
    assert _device_calls(rig.log) == BATCHED and _count(rig.log, "features") == 1
    assert len(_filters(rig.log)) == 1
    used = _filters(rig.log)[0][3]["variance"]
    acc = Accumulator("the scene", camera, moments=True, **rig.kw)
    for _ in range(4):
        acc.add(2)
    assert np.array_equal(_bits(got), _bits(acc.denoised("variance")))
    assert np.array_equal(_bits(used), _bits(acc.moments_state[..., 3]))
    assert np.array_equal(_bits(np.load(tmp_path / "aov" / "variance.npy")), _bits(acc.moments_state[..., 3]))
    # two passes of 4 spp are two batches: below MIN_MOMENT_BATCHES the filter keeps its spatial estimate
    del rig.log[:]
    main(CLI + VARIANCE + ["--interval", "4", "--variance-batches", "4"])
    assert _filters(rig.log)[0][3]["variance"] is None
    # without moments the passes add onto the sums in sample order: render()'s bits
    del rig.log[:]
    got = main(CLI + ["--interval", "3", "--denoise"])
    assert _device_calls(rig.log) == [("accumulate", 0, 3, N_TILES), ("accumulate", 3, 3, N_TILES),
                                      ("accumulate", 6, 2, N_TILES)]
    assert np.array_equal(_bits(got), _bits(_render(rig, camera, "fixed")[0]))


def test_unpack_tiles_takes_any_channel_count():
    from pyrenderer_amd.device_scene import interleaved_tiles, unpack_tiles
    ids = interleaved_tiles(W, H, TILE)
    slots = np.random.default_rng(0).uniform(size=(N_TILES * TILE * TILE, 8)).astype(F32)
    frame = unpack_tiles(slots, W, H, TILE, TILE, ids)
    assert frame.shape == (W, H, 8) and frame.dtype == F32 and np.array_equal(_bits(frame), _bits(_frame_of(slots)))
    for c0 in (0, 3, 5):
        three = unpack_tiles(np.ascontiguousarray(slots[:, c0:c0 + 3]), W, H, TILE, TILE, ids)
        assert np.array_equal(_bits(frame[..., c0:c0 + 3]), _bits(three))
    into = np.full((W, H, 8), F32(-1))
    assert unpack_tiles(slots, W, H, TILE, TILE, ids, into) is into and np.array_equal(_bits(into), _bits(frame))

"""The a-trous denoiser on the GPU: prt_denoise against the NumPy restatement bit for bit, the
device entry point, the feature buffers against the oracle, the quality gain, and the public API."""
import numpy as np
import pytest

import atrous_ref as R
from denoise_cases import bits, gap_soup, hostile_inputs, reference, rmse

pytestmark = pytest.mark.gpu

F32 = np.float32
# non-default parameters for the bit-identity cases, so every term of the weight is at work
PAR = dict(sigma_c=1.5, sigma_z=0.75, eps_a=1e-2, eps_z=2e-3)


_CASES = [(1, 1, 5), (5, 3, 5), (33, 17, 4), (70, 130, 5)]


@pytest.fixture(scope="module")
def restated():
    """Inputs and the restatement's output of every shape, computed once and left unchanged."""
    out = {}
    for W, H, n in _CASES:
        C, F, bad = hostile_inputs(W, H, 100 + W, "uniform")
        out[(W, H)] = (C, F, bad, n, R.atrous(C, F, n, **PAR))
    return out


@pytest.mark.parametrize("W,H", [c[:2] for c in _CASES])
def test_filter_equals_the_restatement_bit_for_bit(restated, W, H):
    from pyrenderer_amd.denoise import denoise
    C, F, bad, n, want = restated[(W, H)]
    got = denoise(C, F, iterations=n, **PAR)
    again = denoise(C, F, iterations=n, **PAR)
    assert np.array_equal(bits(got), bits(again))
    diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
    assert len(diff) == 0, (len(diff), diff[:5])
    ok = np.ones((W, H), bool)
    for x, y in bad:
        ok[x, y] = False
        assert np.array_equal(bits(got[x, y]), bits(C[x, y]))
    assert np.isfinite(got[ok]).all()
    miss = ~(F[..., 7] > 0)
    if W * H > 1:
        assert miss.any() and (~miss).any()
    assert np.array_equal(bits(got[miss]), bits(C[miss]))
    if W * H > 100:   # the filter did something: most surviving hit pixels changed
        assert np.mean(np.any(got[ok & ~miss] != C[ok & ~miss], axis=-1)) > 0.6


@pytest.mark.parametrize("n", [0, 1, 8])
def test_iteration_counts_at_the_ends_of_the_range(restated, n):
    from pyrenderer_amd.denoise import denoise
    C, F, _, _, _ = restated[(33, 17)]
    assert np.array_equal(bits(denoise(C, F, iterations=n, **PAR)), bits(R.atrous(C, F, n, **PAR)))


def test_device_entry_point_on_a_side_stream(restated):
    import torch
    from pyrenderer_amd import denoise as D
    C, F, _, n, want = restated[(70, 130)]
    W, H = C.shape[:2]
    dev = torch.device("cuda:0")
    d_c, d_f = torch.from_numpy(C).to(dev), torch.from_numpy(F).to(dev)
    d_out = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
    need = D.work_bytes(W, H)
    assert need > 0
    d_work = torch.empty(need, dtype=torch.uint8, device=dev)   # exactly the bytes asked for
    assert d_work.data_ptr() % 16 == 0
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    D.denoise_device(d_c.data_ptr(), d_f.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(), need, iterations=n,
                     stream_ptr=stream.cuda_stream, **PAR)
    stream.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(bits(got), bits(D.denoise(C, F, iterations=n, **PAR)))
    assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------- features ----

class _World:
    """features() needs only device_scene() of its world."""

    def __init__(self, ds):
        self.ds = ds

    def device_scene(self, device=0):
        return self.ds


def _expected_features(ds, osc, cam, W, H, tile, samples, seed):
    """The feature buffers without the code under test: the render's primary rays, the oracle's
    hit_all on them, and the same float32 sums in sample order, written pixel by pixel."""
    tx, ty = (W + tile - 1) // tile, (H + tile - 1) // tile
    ids = np.arange(tx * ty, dtype=np.int32)
    o, d, _ = ds.camera_rays(cam, W, H, tile, tile, ids, 0, samples, seed)
    o = o.reshape(samples, tx * ty, tile, tile, 3)
    d = d.reshape(samples, tx * ty, tile, tile, 3)
    acc = np.zeros((W, H, 8), F32)
    for t in ids:
        x0, y0 = (t % tx) * tile, (t // tx) * tile
        w, h = min(tile, W - x0), min(tile, H - y0)
        for s in range(samples):
            ro = o[s, t, :h, :w].reshape(-1, 3)
            rd = d[s, t, :h, :w].reshape(-1, 3)
            assert np.all(np.any(rd != 0, axis=1))
            r = osc.hit_all(ro, rd, 1e-5, 99999.9).reshape(h, w, 16).transpose(1, 0, 2)   # [lx][ly]
            hit = r[..., 0] > 0
            a = acc[x0:x0 + w, y0:y0 + h]
            a[..., 0:3] += r[..., 9:12]
            a[..., 3:6] += r[..., 5:8]
            a[..., 6] += np.where(hit, r[..., 1], F32(0))
            a[..., 7] += hit.astype(F32)
    out = np.zeros((W, H, 8), F32)
    out[..., 0:6] = acc[..., 0:6] / F32(samples)
    out[..., 6] = acc[..., 6] / np.maximum(acc[..., 7], F32(1))
    out[..., 7] = acc[..., 7] / F32(samples)
    return out


@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("which", ["cornell", "soup"])
def test_features_equal_the_oracle_composition(cornell, gpu_scene, oracle_scene, which, samples):
    from oracle import oracle as O
    from pyrenderer_amd.denoise import features
    from pyrenderer_amd.device_scene import DeviceScene
    W, H, tile, seed = 40, 24, 16, 7     # 40 x 24 with 16 x 16 tiles: partial tiles on both edges
    cam = cornell[1]
    if which == "cornell":
        ds, osc = gpu_scene, oracle_scene
    else:
        flat = gap_soup(cornell)
        ds, osc = DeviceScene(flat, 0), O.OracleScene.from_flat(flat)
    got = features(None, cam, resolution=(W, H), samples=samples, seed=seed, tile=tile, world=_World(ds))
    want = _expected_features(ds, osc, cam.convert_to_taichi_camera().packed(), W, H, tile, samples, seed)
    assert got.shape == (W, H, 8) and got.dtype == F32
    assert np.array_equal(bits(got), bits(want)), np.argwhere(np.any(got != want, axis=-1))[:5]
    hit = got[..., 7] > 0
    if which == "soup":
        assert hit.any() and (~hit).any(), (int(hit.sum()), hit.size)
        assert not got[~hit].any()                     # a miss is all zeros
    else:
        assert hit.any()
    if samples == 1:
        assert np.allclose(np.linalg.norm(got[..., 3:6][hit], axis=-1), 1.0, atol=1e-4)
    assert (got[..., 6][hit] > 0).all()
    # a small chunk budget (several tile groups and sample chunks) composes the same bits
    from pyrenderer_amd.denoise import features_packed
    small = features_packed(ds, cam.convert_to_taichi_camera().packed(), W, H, samples=samples, seed=seed, tile=tile,
                            chunk_rays=2 * tile * tile)
    assert np.array_equal(bits(small), bits(got))
    if which == "soup":
        ds.close()


# ----------------------------------------------------------------- quality ----

# RMSE(denoised) / RMSE(noisy) against the 4096-spp render, measured on the MI355X with the default
# parameters (the 128^2, 8-spp columns of the chosen row of profiles/denoise_sweep.txt,
# which are these very frames).  The tests allow sqrt(rho): drift is tolerated, losing half the gain
# in log terms is not.
RHO = {"cornell": 0.4273, "specular": 0.4274}


@pytest.mark.parametrize("which", ["cornell", "specular"])
def test_it_denoises(which):
    from pyrenderer_amd.core.tracing import render
    from pyrenderer_amd.denoise import denoise, features
    scene, cam, world, ref = reference(which)
    res = (128, 128)
    noisy = render(scene, cam, spp=8, depth=8, seed=2, resolution=res, world=world)
    feat = features(scene, cam, resolution=res, samples=1, seed=2, world=world)
    den = denoise(noisy, feat)
    e_noisy, e_den = rmse(noisy, ref), rmse(den, ref)
    print(f"denoise quality {which}: rmse noisy {e_noisy:.6f} denoised {e_den:.6f} ratio {e_den / e_noisy:.4f}")
    assert np.isfinite(den).all()
    assert e_den < e_noisy, (e_den, e_noisy)
    assert e_den / e_noisy <= np.sqrt(RHO[which]), (e_den / e_noisy, RHO[which])


# -------------------------------------------------------------- public API ----

def test_public_entry_points_agree(cornell):
    from pyrenderer_amd.core.tracing import Accumulator, build_world, render
    from pyrenderer_amd.denoise import denoise, features
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    kw = dict(depth=4, seed=3, resolution=(48, 40), world=world)
    plain = render(scene, cam, spp=4, **kw)
    assert np.array_equal(bits(render(scene, cam, spp=4, denoise=False, **kw)), bits(plain))
    a = render(scene, cam, spp=4, denoise=True, **kw)
    b = denoise(plain, features(scene, cam, resolution=(48, 40), samples=1, seed=3, world=world))
    acc = Accumulator(scene, cam, **kw)
    acc.add(3).add(1)
    c = acc.denoised()
    assert np.array_equal(bits(acc.mean()), bits(plain))
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    assert not np.array_equal(a, plain) and np.isfinite(a).all()

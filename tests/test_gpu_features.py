"""features_kernel (prt_features / prt_features_device) against the host composition it replaces
(denoise.features_packed_host: prt_camera_rays, prt_hit_all and float32 sums in sample order), bit for
bit on every pixel and channel; the device entry point's bounds, argument errors and watchdog; and the
device chain render -> scatter -> features -> filter against render(denoise=...)."""
import copy

import numpy as np
import pytest

from denoise_cases import bits, gap_soup, load_scene
from kernel_parity import packed_camera

pytestmark = pytest.mark.gpu

F32 = np.float32
TILE = 16            # the host composition's tile: partial 16-pixel tiles on both edges of 40 x 24
W0, H0 = 40, 24
PRT_ERR_ARG = -1


def _same(got, want):
    assert got.shape == want.shape and got.dtype == F32
    diff = np.argwhere(np.any(bits(got) != bits(want), axis=-1))
    assert len(diff) == 0, (len(diff), diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def _host(ds, cam, W, H, samples, seed, first_sample=0):
    from pyrenderer_amd.denoise import features_packed_host
    return features_packed_host(ds, cam, W, H, samples=samples, seed=seed, tile=TILE, first_sample=first_sample)


@pytest.fixture(scope="module")
def packed(cornell):
    return packed_camera(cornell)


# ------------------------------------------------------------ bit equality ----

@pytest.mark.parametrize("samples,first", [(1, 0), (3, 0), (3, 5)])
def test_cornell_ragged_frame(gpu_scene, packed, samples, first):
    got = gpu_scene.features(packed, W0, H0, samples=samples, first_sample=first, seed=7)
    _same(got, _host(gpu_scene, packed, W0, H0, samples, 7, first))
    assert (got[..., 7] > 0).any()
    gpu_scene.check_faults()
    if first == 0:   # the public front end is the same call
        from pyrenderer_amd.denoise import features_packed
        _same(features_packed(gpu_scene, packed, W0, H0, samples=samples, seed=7, tile=TILE, chunk_rays=512), got)


@pytest.mark.parametrize("samples", [1, 3])
def test_gap_soup_has_hits_and_all_zero_misses(cornell, packed, samples):
    from pyrenderer_amd.device_scene import DeviceScene
    ds = DeviceScene(gap_soup(cornell), 0)
    got = ds.features(packed, W0, H0, samples=samples, seed=7)
    _same(got, _host(ds, packed, W0, H0, samples, 7))
    hit = got[..., 7] > 0
    assert hit.any() and (~hit).any(), (int(hit.sum()), hit.size)
    assert not bits(got[~hit]).any()          # every miss pixel is all +0.0 bits
    ds.check_faults()
    ds.close()


def test_specular_scene_with_a_sphere():
    """scene_specular.json at 48 x 48, 2 samples: metal / dielectric rows and a sphere.  With seed 7 the
    CPU oracle's closest hits on the host gen_ray rays of this frame put 253 of the 4608 primary rays on
    the sphere (hit id >= n_tri = 36), so neither the frame nor the seed needed changing."""
    from pyrenderer_amd.device_scene import DeviceScene
    from pyrenderer_amd.flatten import flatten_scene
    scene, cam = load_scene("specular")
    flat = flatten_scene(scene)
    pc = cam.convert_to_taichi_camera().packed()
    ds = DeviceScene(flat, 0)
    W = H = 48
    ids = np.arange(9, dtype=np.int32)
    o, dd, _ = ds.camera_rays(pc, W, H, TILE, TILE, ids, 0, 2, 7)
    hid, _ = ds.closest_hits(o, dd, 1e-5, 99999.9)
    assert (hid >= flat.n_tri).any()
    assert set(flat.mat[:, 5]) >= {2.0, 3.0}   # metal and dielectric material rows
    _same(ds.features(pc, W, H, samples=2, seed=7), _host(ds, pc, W, H, 2, 7))
    ds.check_faults()
    ds.close()


@pytest.mark.parametrize("mod", ["aperture", "projective"])
def test_thin_lens_and_projective_cameras(gpu_scene, cornell, mod):
    pc = copy.deepcopy(cornell[1].convert_to_taichi_camera())
    if mod == "aperture":
        pc.sensor_dim = pc.sensor_dim.copy()
        pc.sensor_dim[3] = F32(1.0)
    else:
        pc.iview_cols = pc.iview_cols.copy()
        pc.iview_cols[3, 0] = F32(1e-3)
    cam = pc.packed()
    got = gpu_scene.features(cam, W0, H0, samples=2, seed=7)
    _same(got, _host(gpu_scene, cam, W0, H0, 2, 7))
    assert (got[..., 7] > 0).any()
    gpu_scene.check_faults()


def test_global_scene_f32_and_quantised_nodes():
    from pyrenderer_amd import scenes
    from pyrenderer_amd.device_scene import DeviceScene
    from pyrenderer_amd.flatten import flatten_scene
    scene, cam = scenes.instanced_cubes(n_instances=2000)
    ds = DeviceScene(flatten_scene(scene), 0)
    assert not ds.kernel_info()["lds_scene"]
    pc = cam.convert_to_taichi_camera().packed()
    W, H = 48, 32
    plain = ds.features(pc, W, H, samples=2, seed=7)
    quant = ds.features(pc, W, H, samples=2, seed=7, quantized=True)
    _same(quant, plain)
    _same(plain, _host(ds, pc, W, H, 2, 7))
    ds.check_faults()
    ds.close()


def test_the_high_seed_word_reaches_the_key(gpu_scene, packed):
    seed = 2 ** 40 + 7
    got = gpu_scene.features(packed, W0, H0, seed=seed)
    _same(got, _host(gpu_scene, packed, W0, H0, 1, seed))
    assert not np.array_equal(bits(got), bits(gpu_scene.features(packed, W0, H0, seed=7)))
    gpu_scene.check_faults()


# ------------------------------------------------- the device entry point ----

NAN_BITS = 0x7FC0BEEF


@pytest.mark.parametrize("W,H", [(1, 1), (65, 1), (1, 65), (72, 40)])
def test_degenerate_frames_stay_inside_their_buffer(gpu_scene, packed, W, H):
    """prt_features_device writes W * H * 8 floats and nothing else: 64 floats before the output pointer and
    64 after the body keep a fixed NaN pattern; the body is prt_features' output."""
    import torch
    dev = torch.device("cuda:0")
    n = W * H * 8
    buf = torch.full((64 + n + 64,), NAN_BITS, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    gpu_scene.features_device(packed, W, H, buf.data_ptr() + 64 * 4, samples=1, seed=7, stream_ptr=stream.cuda_stream)
    stream.synchronize()
    gpu_scene.check_faults()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:64] == NAN_BITS).all() and (got[64 + n:] == NAN_BITS).all()
    want = gpu_scene.features(packed, W, H, samples=1, seed=7)
    assert np.array_equal(got[64:64 + n], bits(want).reshape(-1))
    gpu_scene.check_faults()


@pytest.mark.parametrize("case", ["samples0", "first_neg", "flags_any", "w0"])
def test_argument_errors(gpu_scene, packed, case):
    from pyrenderer_amd import _native as N
    W, H, first, samples, flags = W0, H0, 0, 1, 0
    if case == "samples0":
        samples = 0
    elif case == "first_neg":
        first = -1
    elif case == "flags_any":
        flags = N.PRT_HITS_ANY
    else:
        W = 0
    out = np.zeros((max(W, 1), H, 8), F32)
    with pytest.raises(N.PrtError) as e:
        N.check(N.lib().prt_features(gpu_scene.h, N.ptr(packed), W, H, first, samples, 7, flags, N.ptr(out)))
    assert e.value.code == PRT_ERR_ARG
    with pytest.raises(N.PrtError) as e:
        N.check(N.lib().prt_features_device(gpu_scene.h, N.ptr(packed), W, H, first, samples, 7, flags, 4096, None))
    assert e.value.code == PRT_ERR_ARG
    assert not out.any()
    gpu_scene.check_faults()


# -------------------------------------------------------- the device chain ----

@pytest.mark.parametrize("mode", ["fixed", "variance"])
def test_device_chain_equals_the_filtered_render(cornell, mode):
    """render_tiles_device -> scatter_tiles -> / 8 -> features_device -> denoise*_device on one torch stream,
    no host copy in between, against render(denoise=...) of the same frame."""
    import torch
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import build_world, render
    from pyrenderer_amd.device_scene import interleaved_tiles
    scene, cam, _ = cornell
    world = build_world(scene, (0,))
    W, H, tile, spp, depth, seed = 72, 40, 64, 8, 4, 3
    want = render(scene, cam, spp=spp, depth=depth, seed=seed, resolution=(W, H), tile=tile, world=world,
                  denoise=True if mode == "fixed" else "variance")
    ds = world.device_scene(0)
    pc = cam.convert_to_taichi_camera().packed()
    ids = interleaved_tiles(W, H, tile)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        d_packed = torch.zeros((ids.shape[0] * tile * tile, 3), dtype=torch.float32, device=dev)
        d_sums = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
        d_feat = torch.zeros((W, H, 8), dtype=torch.float32, device=dev)
        d_out = torch.zeros((W, H, 3), dtype=torch.float32, device=dev)
        need = D.work_bytes_variance(W, H) if mode == "variance" else D.work_bytes(W, H)
        d_work = torch.empty(need, dtype=torch.uint8, device=dev)
        sp = stream.cuda_stream
        ds.render_tiles_device(pc, W, H, tile, tile, ids, spp, depth, d_packed.data_ptr(), stream_ptr=sp, seed=seed)
        ds.scatter_tiles(d_packed.data_ptr(), ids, tile, tile, W, H, d_sums.data_ptr(), stream_ptr=sp)
        d_mean = d_sums / F32(spp)
        D.features_device(ds, pc, W, H, d_feat.data_ptr(), samples=1, seed=seed, stream_ptr=sp)
        if mode == "variance":
            D.denoise_variance_device(d_mean.data_ptr(), d_feat.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(),
                                      need, stream_ptr=sp)
        else:
            D.denoise_device(d_mean.data_ptr(), d_feat.data_ptr(), W, H, d_out.data_ptr(), d_work.data_ptr(), need,
                             stream_ptr=sp)
    stream.synchronize()
    ds.check_faults()
    got = d_out.cpu().numpy()
    _same(got, want)
    assert np.isfinite(got).all() and got.any()

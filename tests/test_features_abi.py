"""prt_features / prt_features_device without a GPU: declared, exported and bound under ABI 4; a NULL
scene is rejected before any device is touched, with a text in prt_last_error; the Python front ends
keep their signatures."""
import inspect
import os
import re

import numpy as np

from conftest import ROOT

NAMES = ("prt_features", "prt_features_device")
PRT_ERR_ARG = -1
FAKE = 4096   # a device "pointer" that is never dereferenced: the checks fail first


def _header():
    return open(os.path.join(ROOT, "include", "prt.h")).read()


def test_header_and_exports_carry_the_entry_points():
    from pyrenderer_amd import _native as N
    src = _header()
    declared = set(re.findall(r"\b(prt_[a-z_0-9]+)\s*\(", src))
    L = N.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in N.EXPORTS, n
        assert hasattr(L, n), n
    assert re.search(r"^#define PRT_FEATURE_CHANNELS 8$", src, re.M)
    assert L.prt_abi_version() == 4 and "#define PRT_ABI_VERSION 4" in src


def test_the_symbols_are_in_the_shared_library():
    import ctypes
    from pyrenderer_amd.build import LIB
    raw = ctypes.CDLL(LIB)     # no bindings: the dynamic symbol table itself
    for n in NAMES:
        assert getattr(raw, n) is not None, n


def test_a_null_scene_is_rejected_with_a_message():
    from pyrenderer_amd import _native as N
    L = N.lib()
    cam = np.zeros(24, np.float32)
    out = np.zeros((4, 3, 8), np.float32)
    import ctypes
    h = ctypes.c_void_p()
    assert L.prt_bvh_build(None, 5, 4, ctypes.byref(h)) == PRT_ERR_ARG   # leaves another text behind
    before = L.prt_last_error()
    assert L.prt_features(None, N.ptr(cam), 4, 3, 0, 1, 0, 0, N.ptr(out)) == PRT_ERR_ARG
    msg = L.prt_last_error()
    assert msg and msg != before and b"scene" in msg
    assert not out.any()
    assert L.prt_bvh_build(None, 5, 4, ctypes.byref(h)) == PRT_ERR_ARG
    assert L.prt_features_device(None, N.ptr(cam), 4, 3, 0, 1, 0, 0, FAKE, None) == PRT_ERR_ARG
    msg = L.prt_last_error()
    assert msg and msg != before and b"scene" in msg


def test_python_front_ends():
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.device_scene import DeviceScene
    p = inspect.signature(D.features_packed).parameters
    assert list(p)[:4] == ["ds", "cam_packed", "W", "H"]
    assert {"samples", "seed", "tile", "chunk_rays"} <= set(p)          # both still accepted
    assert "no longer affect" in D.features_packed.__doc__
    h = inspect.signature(D.features_packed_host).parameters
    assert set(p) | {"first_sample"} == set(h) and h["first_sample"].default == 0
    assert "slow path" in D.features_packed_host.__doc__
    assert list(inspect.signature(D.features_device).parameters)[:5] == ["ds", "cam_packed", "W", "H", "d_out_ptr"]
    f = inspect.signature(DeviceScene.features).parameters
    assert [(k, v.default) for k, v in f.items()][4:] == [("samples", 1), ("first_sample", 0), ("seed", 0),
                                                          ("quantized", False)]
    g = inspect.signature(DeviceScene.features_device).parameters
    assert list(g)[1:5] == ["cam", "W", "H", "d_out_ptr"] and g["stream_ptr"].default is None
    assert D.FEATURE_CHANNELS == 8


def test_features_packed_calls_the_kernel_and_ignores_tile_and_chunk():
    """features_packed is ds.features(...): one call, whatever tile and chunk_rays say."""
    from pyrenderer_amd import denoise as D

    class Ds:
        calls = []

        def features(self, cam, W, H, samples=1, first_sample=0, seed=0, quantized=False):
            self.calls.append((W, H, samples, first_sample, seed, quantized))
            return np.zeros((W, H, 8), np.float32)

    ds = Ds()
    cam = np.zeros(24, np.float32)
    a = D.features_packed(ds, cam, 5, 3, samples=2, seed=9)
    D.features_packed(ds, cam, 5, 3, samples=2, seed=9, tile=16, chunk_rays=512)
    assert a.shape == (5, 3, 8) and ds.calls == [(5, 3, 2, 0, 9, False)] * 2

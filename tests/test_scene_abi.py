"""prt_scene_create's argument checks through the C ABI, on a machine without a GPU: every rejected
scene returns PRT_ERR_ARG with its message before any device is touched (tests/scene_cases.py holds
the cases; tests/test_host_plan.py runs the same ones against the sanitizer build of the checks)."""
import ctypes

import pytest

from pyrenderer_amd import _native as N
from scene_cases import REJECTED, base_scene

PRT_ERR_ARG, PRT_ERR_HIP = -1, -2


def _create(s, with_out=True):
    L = N.lib()
    h = ctypes.c_void_p()
    rc = L.prt_scene_create(0, N.ptr(s["tri_v"]), N.ptr(s["tri_n"]), N.ptr(s["tri_mat"]), s["n_tri"], N.ptr(s["sph"]),
                            N.ptr(s["sph_mat"]), s["n_sph"], N.ptr(s["mat"]), s["n_mat"], N.ptr(s["light_tri"]),
                            N.ptr(s["light_off"]), s["n_light"], None, ctypes.byref(h) if with_out else None)
    return rc, L.prt_last_error().decode(), h


@pytest.mark.parametrize("name,args,message", REJECTED, ids=[c[0] for c in REJECTED])
def test_rejected_scene_reports_its_first_failed_check(name, args, message):
    rc, err, h = _create(args)
    assert (rc, err) == (PRT_ERR_ARG, message)
    assert not h.value


def test_missing_out_pointer_is_rejected_first():
    bad = dict(base_scene(), n_tri=-1)
    assert _create(bad, with_out=False)[:2] == (PRT_ERR_ARG, "out_scene is NULL")


def test_valid_scene_needs_a_device():
    if N.device_count() > 0:
        pytest.skip("a HIP device is present: the scene is created (GPU suite)")
    rc, err, h = _create(base_scene())
    assert (rc, err) == (PRT_ERR_HIP, "no HIP device available")
    assert not h.value

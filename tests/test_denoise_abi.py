"""The denoiser's C-ABI without a GPU: the four entry points are declared, exported and bound, and
prt_denoise rejects bad arguments before touching a device, with its own error text."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("prt_denoise", "prt_denoise_device", "prt_denoise_work_bytes", "prt_denoise_last_error")


def test_header_and_exports_carry_the_denoise_entry_points():
    from pyrenderer_amd import _native as N
    src = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z_0-9]+)\s*\(", src))
    L = N.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in N.EXPORTS, n
        assert hasattr(L, n), n
    assert L.prt_abi_version() == 4


def test_denoise_sources_are_outside_the_kernel_hash():
    """The new units are build dependencies but do not key the counter profiles."""
    from pyrenderer_amd import build as B
    assert set(B.AUX_SOURCES) == {"prt_denoise.hip", "prt_denoise_capi.cpp"}
    hashed = set(B.SOURCES + B.HEADERS + [B.TRACE_INST])
    assert not hashed & set(B.AUX_SOURCES + B.AUX_HEADERS)
    for f in B.AUX_SOURCES + B.AUX_HEADERS:
        assert os.path.exists(os.path.join(B.CSRC, f)), f


def _call(color, feat, W, H, iterations, params, out, device=0):
    from pyrenderer_amd import _native as N
    L = N.lib()
    rc = L.prt_denoise(device, N.ptr(color), N.ptr(feat), W, H, iterations, N.ptr(params), N.ptr(out))
    return rc, L.prt_denoise_last_error()


GOOD = (1.0, 1.0, 1e-2, 1e-3)


@pytest.mark.parametrize("case,word", [
    ("null_color", b"NULL"), ("null_feat", b"NULL"), ("null_out", b"NULL"), ("null_params", b"NULL"),
    ("w0", b"W and H"), ("h0", b"W and H"), ("h_huge", b"W and H"), ("iter9", b"iterations"), ("iter_neg", b"iterations"),
    ("sigma_c0", b"sigma"), ("sigma_z_neg", b"sigma"), ("sigma_nan", b"sigma"), ("eps_a0", b"eps"),
    ("eps_z_inf", b"eps"), ("sigma_c_tiny", b"sigma_c squared"),
])
def test_bad_arguments_are_rejected_before_any_device(case, word):
    W, H, it = 4, 3, 5
    color = np.zeros((W, H, 3), np.float32)
    feat = np.zeros((W, H, 8), np.float32)
    out = np.zeros((W, H, 3), np.float32)
    par = np.array(GOOD, np.float32)
    if case == "null_color":
        color = None
    elif case == "null_feat":
        feat = None
    elif case == "null_out":
        out = None
    elif case == "null_params":
        par = None
    elif case == "w0":
        W = 0
    elif case == "h0":
        H = 0
    elif case == "h_huge":
        H = 32769
    elif case == "iter9":
        it = 9
    elif case == "iter_neg":
        it = -1
    elif case == "sigma_c0":
        par[0] = 0.0
    elif case == "sigma_z_neg":
        par[1] = -1.0
    elif case == "sigma_nan":
        par[0] = np.nan
    elif case == "eps_a0":
        par[2] = 0.0
    elif case == "eps_z_inf":
        par[3] = np.inf
    elif case == "sigma_c_tiny":
        par[0] = 1e-22
    rc, msg = _call(color, feat, W, H, it, par, out)
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(b"prt_denoise:") and word in msg, msg


def test_device_entry_point_checks_its_scratch_without_a_gpu():
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H = 70, 130
    need = L.prt_denoise_work_bytes(W, H)
    assert need >= W * H * 56 and need % 256 == 0
    assert L.prt_denoise_work_bytes(0, 4) == 0
    par = np.array(GOOD, np.float32)
    fake = 4096   # never dereferenced: the checks fail first
    assert L.prt_denoise_device(0, fake, fake, W, H, 5, N.ptr(par), fake * 2, fake * 3, need - 1, None) == -1
    assert b"prt_denoise_work_bytes" in L.prt_denoise_last_error()
    assert L.prt_denoise_device(0, fake, fake, W, H, 5, N.ptr(par), fake * 2, fake * 3 + 4, need, None) == -1
    assert b"aligned" in L.prt_denoise_last_error()
    assert L.prt_denoise_device(0, None, fake, W, H, 5, N.ptr(par), fake * 2, fake * 3, need, None) == -1
    assert b"NULL" in L.prt_denoise_last_error()


def test_python_wrapper_raises_with_the_denoisers_text():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.denoise import denoise
    with pytest.raises(N.PrtError, match="iterations"):
        denoise(np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32), iterations=9)
    with pytest.raises(ValueError):
        denoise(np.zeros((2, 2, 3), np.float32), np.zeros((2, 3, 8), np.float32))

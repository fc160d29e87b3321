"""The variance-guided denoiser's C-ABI and front ends without a GPU: the three entry points are
declared, exported and bound, bad arguments are rejected before any device is touched with the
denoiser's own error text, and the Python and command-line switches parse."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("prt_denoise_var", "prt_denoise_var_device", "prt_denoise_var_work_bytes")
GOOD = (1.0, 2.0, 1e-2, 1e-2, 1e-2)   # sigma_l, sigma_z, eps_a, eps_z, eps_l
PARAM_NAMES = ("sigma_l", "sigma_z", "eps_a", "eps_z", "eps_l")


def test_header_and_exports_carry_the_entry_points():
    from pyrenderer_amd import _native as N
    src = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z_0-9]+)\s*\(", src))
    L = N.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in N.EXPORTS, n
        assert hasattr(L, n), n
    assert L.prt_abi_version() == 4
    assert "#define PRT_ABI_VERSION 4" in src


def _call(color, feat, W, H, iterations, params, out, var=None, device=0):
    from pyrenderer_amd import _native as N
    L = N.lib()
    rc = L.prt_denoise_var(device, N.ptr(color), N.ptr(feat), W, H, iterations, N.ptr(params), N.ptr(out), N.ptr(var))
    return rc, L.prt_denoise_last_error()


_BAD_VALUES = {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf}
_CASES = [("null_color", b"NULL"), ("null_feat", b"NULL"), ("null_out", b"NULL"), ("null_params", b"NULL"),
          ("w0", b"W and H"), ("h0", b"W and H"), ("w_huge", b"W and H"), ("h_huge", b"W and H"),
          ("iter9", b"iterations"), ("iter_neg", b"iterations")]
_CASES += [(f"{name}:{how}", name.encode()) for name in PARAM_NAMES for how in _BAD_VALUES]


@pytest.mark.parametrize("case,word", _CASES)
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
    elif case == "w_huge":
        W = 32769
    elif case == "h_huge":
        H = 32769
    elif case == "iter9":
        it = 9
    elif case == "iter_neg":
        it = -1
    else:
        name, how = case.split(":")
        par[PARAM_NAMES.index(name)] = _BAD_VALUES[how]
    rc, msg = _call(color, feat, W, H, it, par, out)
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(b"prt_denoise_var:") and word in msg, msg


def test_device_entry_point_checks_its_scratch_without_a_gpu():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.denoise import work_bytes_variance
    L = N.lib()
    W, H = 70, 130
    need = L.prt_denoise_var_work_bytes(W, H)
    assert need >= W * H * 60 and need % 256 == 0 and need == work_bytes_variance(W, H)
    assert L.prt_denoise_var_work_bytes(0, 4) == 0 and L.prt_denoise_var_work_bytes(4, 32769) == 0
    par = np.array(GOOD, np.float32)
    fake = 4096   # never dereferenced: the checks fail first

    def dev(color=fake, out=fake * 2, var=None, work=fake * 3, size=need, params=par):
        rc = L.prt_denoise_var_device(0, color, fake * 5, W, H, 5, N.ptr(params), out, var, work, size, None)
        return rc, L.prt_denoise_last_error()

    rc, msg = dev(size=need - 1)
    assert rc == -1 and b"prt_denoise_var_work_bytes" in msg, msg
    rc, msg = dev(work=fake * 3 + 4)
    assert rc == -1 and b"aligned" in msg, msg
    rc, msg = dev(color=None)
    assert rc == -1 and b"NULL" in msg, msg
    rc, msg = dev(work=None)
    assert rc == -1 and b"NULL" in msg, msg
    rc, msg = dev(out=fake)
    assert rc == -1 and b"alias" in msg, msg
    for var in (fake, fake * 2, fake * 5):   # the variance plane on the colour, the output, the features
        rc, msg = dev(var=var)
        assert rc == -1 and b"alias" in msg and b"d_out_var" in msg, msg
    bad = par.copy()
    bad[4] = 0.0
    rc, msg = dev(params=bad)
    assert rc == -1 and msg.startswith(b"prt_denoise_var_device:") and b"eps_l" in msg, msg


def test_python_wrapper_raises_with_the_denoisers_text():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.denoise import denoise_variance
    c, f = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32)
    with pytest.raises(N.PrtError, match="prt_denoise_var: iterations"):
        denoise_variance(c, f, iterations=9)
    with pytest.raises(N.PrtError, match="sigma_l"):
        denoise_variance(c, f, sigma_l=0.0, return_variance=True)
    with pytest.raises(ValueError):
        denoise_variance(c, np.zeros((2, 3, 8), np.float32))


def test_module_constants_are_the_documented_defaults():
    import inspect
    from pyrenderer_amd import denoise as D
    sig = inspect.signature(D.denoise_variance).parameters
    assert sig["sigma_l"].default == D.VAR_SIGMA_L and sig["eps_l"].default == D.VAR_EPS_L
    assert sig["sigma_z"].default == D.VAR_SIGMA_Z and sig["eps_a"].default == D.EPS_A
    assert sig["eps_z"].default == D.EPS_Z and sig["iterations"].default == D.ITERATIONS
    assert sig["return_variance"].default is False
    assert D.MODES == ("fixed", "variance")


def test_render_rejects_an_unknown_denoise_mode():
    from pyrenderer_amd.core.tracing import Accumulator, render
    for bad in ("nonsense", "fixed", 1, None):
        with pytest.raises(ValueError, match="denoise"):
            render(None, None, spp=1, depth=1, denoise=bad)
    assert "mode" in Accumulator.denoised.__code__.co_varnames


def test_denoise_mode_flag():
    from pyrenderer_amd import main as M
    assert M.parse([]).denoise_mode == "fixed"
    assert M.parse(["--denoise"]).denoise_mode == "fixed"
    a = M.parse(["--denoise", "--denoise-mode", "variance", "--aov", "aov/"])
    assert a.denoise is True and a.denoise_mode == "variance" and a.aov == "aov/"
    assert M.parse(["--denoise", "--denoise-mode", "fixed"]).denoise_mode == "fixed"


@pytest.mark.parametrize("word", ["svgf", "Variance", ""])
def test_an_unknown_denoise_mode_is_a_usage_error(word, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.parse(["--denoise", "--denoise-mode", word])
    assert e.value.code == 2
    assert "--denoise-mode" in capsys.readouterr().err

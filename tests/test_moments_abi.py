"""The sample-moments entry points and their front ends without a GPU: declared, exported and bound;
bad arguments rejected before any device is touched, with the denoiser's own error text; the Python
ValueErrors and the --variance-batches switch."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("prt_moments_add", "prt_moments_add_device", "prt_denoise_var_given", "prt_denoise_var_given_device")
GOOD = (1.0, 2.0, 1e-2, 1e-2, 1e-2)   # sigma_l, sigma_z, eps_a, eps_z, eps_l
PARAM_NAMES = ("sigma_l", "sigma_z", "eps_a", "eps_z", "eps_l")
_BAD_VALUES = {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf}
FAKE = 4096   # a device "pointer" that is never dereferenced: the checks fail first


def test_header_and_exports_carry_the_entry_points():
    from pyrenderer_amd import _native as N
    src = open(os.path.join(ROOT, "include", "prt.h")).read()
    declared = set(re.findall(r"\b(prt_[a-z_0-9]+)\s*\(", src))
    L = N.lib()
    for n in NAMES:
        assert n in declared, n
        assert n in N.EXPORTS, n
        assert hasattr(L, n), n
    assert L.prt_abi_version() == 4 and "#define PRT_ABI_VERSION 4" in src


def test_the_trace_kernels_key_is_unchanged():
    """Nothing in SOURCES, HEADERS, TRACE_INST, FLAGS or UNIT_FLAGS changed: profiles/pmc.json stays valid."""
    import json
    from pyrenderer_amd import build as B
    assert "prt_denoise.hip" in B.AUX_SOURCES and "prt_denoise.hip" not in B.SOURCES
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
    assert B.kernel_sha() in json.dumps(pmc)


# ------------------------------------------------------------ prt_moments_add ----

_M_CASES = [("null_sums", b"NULL"), ("null_feat", b"NULL"), ("null_state", b"NULL"),
            ("w0", b"W and H"), ("h0", b"W and H"), ("w_huge", b"W and H"), ("h_huge", b"W and H"),
            ("frames0", b"n_frames"), ("frames_neg", b"n_frames"), ("pitch_short", b"frame_pitch"),
            ("pitch_neg", b"frame_pitch"), ("n0", b"n_samples"), ("n_half", b"n_samples"), ("n_nan", b"n_samples"),
            ("n_inf", b"n_samples"), ("n_neg", b"n_samples")]
_M_CASES += [(f"eps_a:{how}", b"eps_a") for how in _BAD_VALUES]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _M_CASES)
def test_moments_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H, nf, pitch, n, eps_a = 4, 3, 2, 0, 2.0, 1e-2
    sums = np.zeros((nf, W, H, 3), np.float32)
    feat = np.zeros((W, H, 8), np.float32)
    state = np.zeros((W, H, 4), np.float32)
    p_sums, p_feat, p_state = (FAKE, FAKE * 2, FAKE * 3) if device_form else (N.ptr(sums), N.ptr(feat), N.ptr(state))
    if case == "null_sums":
        p_sums = None
    elif case == "null_feat":
        p_feat = None
    elif case == "null_state":
        p_state = None
    elif case == "w0":
        W = 0
    elif case == "h0":
        H = 0
    elif case == "w_huge":
        W = 32769
    elif case == "h_huge":
        H = 32769
    elif case == "frames0":
        nf = 0
    elif case == "frames_neg":
        nf = -1
    elif case == "pitch_short":
        pitch = W * H * 3 - 1
    elif case == "pitch_neg":
        pitch = -(W * H * 3)
    elif case.startswith("n"):
        n = {"n0": 0.0, "n_half": 0.5, "n_nan": np.nan, "n_inf": np.inf, "n_neg": -4.0}[case]
    else:
        eps_a = _BAD_VALUES[case.split(":")[1]]
    if device_form:
        rc = L.prt_moments_add_device(0, p_sums, nf, pitch, n, p_feat, eps_a, W, H, p_state, None)
        who = b"prt_moments_add_device:"
    else:
        rc = L.prt_moments_add(0, p_sums, nf, pitch, n, p_feat, eps_a, W, H, p_state)
        who = b"prt_moments_add:"
    msg = L.prt_denoise_last_error()
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(who) and word in msg, msg
    assert not state.any()


def test_moments_device_form_wants_an_aligned_state():
    from pyrenderer_amd import _native as N
    L = N.lib()
    rc = L.prt_moments_add_device(0, FAKE, 1, 0, 1.0, FAKE * 2, 1e-2, 4, 3, FAKE * 3 + 4, None)
    assert rc == -1 and b"aligned" in L.prt_denoise_last_error()


# ------------------------------------------------------ prt_denoise_var_given ----

_G_CASES = [("null_color", b"NULL"), ("null_feat", b"NULL"), ("null_in_var", b"NULL"), ("null_out", b"NULL"),
            ("null_params", b"NULL"), ("w0", b"W and H"), ("h0", b"W and H"), ("w_huge", b"W and H"),
            ("h_huge", b"W and H"), ("iter9", b"iterations"), ("iter_neg", b"iterations")]
_G_CASES += [(f"{name}:{how}", name.encode()) for name in PARAM_NAMES for how in _BAD_VALUES]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _G_CASES)
def test_given_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H, it = 4, 3, 5
    color = np.zeros((W, H, 3), np.float32)
    feat = np.zeros((W, H, 8), np.float32)
    in_var = np.zeros((W, H), np.float32)
    out = np.zeros((W, H, 3), np.float32)
    par = np.array(GOOD, np.float32)
    if device_form:
        p = dict(color=FAKE, feat=FAKE * 2, in_var=FAKE * 3, out=FAKE * 4)
    else:
        p = dict(color=N.ptr(color), feat=N.ptr(feat), in_var=N.ptr(in_var), out=N.ptr(out))
    if case.startswith("null_") and case != "null_params":
        p[case[5:]] = None
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
    if device_form:
        rc = L.prt_denoise_var_given_device(0, p["color"], p["feat"], p["in_var"], W, H, it, N.ptr(par), p["out"], None,
                                            FAKE * 8, 1 << 40, None)
        who = b"prt_denoise_var_given_device:"
    else:
        rc = L.prt_denoise_var_given(0, p["color"], p["feat"], p["in_var"], W, H, it, N.ptr(par), p["out"], None)
        who = b"prt_denoise_var_given:"
    msg = L.prt_denoise_last_error()
    assert rc == -1, (rc, msg)
    assert msg.startswith(who) and word in msg, msg


def test_given_device_form_checks_scratch_and_aliasing_without_a_gpu():
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H = 70, 130
    need = L.prt_denoise_var_work_bytes(W, H)   # no new scratch: the spatial mode's 60 B per pixel
    par = np.array(GOOD, np.float32)

    def dev(color=FAKE, in_var=FAKE * 7, out=FAKE * 2, var=None, work=FAKE * 3, size=need):
        rc = L.prt_denoise_var_given_device(0, color, FAKE * 5, in_var, W, H, 5, N.ptr(par), out, var, work, size, None)
        return rc, L.prt_denoise_last_error()

    rc, msg = dev(size=need - 1)
    assert rc == -1 and b"prt_denoise_var_work_bytes" in msg, msg
    rc, msg = dev(work=FAKE * 3 + 4)
    assert rc == -1 and b"aligned" in msg, msg
    rc, msg = dev(work=None)
    assert rc == -1 and b"NULL" in msg, msg
    rc, msg = dev(out=FAKE)
    assert rc == -1 and b"alias" in msg, msg
    rc, msg = dev(in_var=FAKE * 2)
    assert rc == -1 and b"alias" in msg and b"d_in_var" in msg, msg
    rc, msg = dev(in_var=FAKE * 9, var=FAKE * 9)
    assert rc == -1 and b"alias" in msg and b"d_in_var" in msg, msg
    for var in (FAKE, FAKE * 2, FAKE * 5):
        rc, msg = dev(var=var)
        assert rc == -1 and b"alias" in msg and b"d_out_var" in msg, msg


# ------------------------------------------------------------------ Python ----

def test_python_wrappers_raise():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd import denoise as D
    c, f = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32)
    with pytest.raises(ValueError, match="variance must be"):
        D.denoise_variance(c, f, variance=np.zeros((2, 3), np.float32))
    with pytest.raises(N.PrtError, match="prt_denoise_var_given: iterations"):
        D.denoise_variance(c, f, iterations=9, variance=np.zeros((2, 2), np.float32))
    st = D.moments_state(2, 2)
    assert st.shape == (2, 2, 4) and st.dtype == np.float32 and not st.any()
    with pytest.raises(N.PrtError, match="prt_moments_add: n_samples"):
        D.moments_add(st, c, 0, f)
    with pytest.raises(N.PrtError, match="prt_moments_add: eps_a"):
        D.moments_add(st, c[None], 4, f, eps_a=0.0)
    with pytest.raises(ValueError, match="sums_frames"):
        D.moments_add(st, np.zeros((1, 2, 3, 3), np.float32), 4, f)
    with pytest.raises(ValueError, match="state"):
        D.moments_add(np.zeros((2, 2, 4), np.float64), c, 4, f)
    with pytest.raises(ValueError, match="feat"):
        D.moments_add(st, c, 4, np.zeros((2, 2, 7), np.float32))
    with pytest.raises(N.PrtError, match="prt_moments_add_device: n_frames"):
        D.moments_add_device(FAKE, 0, 4, FAKE * 2, 2, 2, FAKE * 3)


def test_constants_and_signatures():
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import Accumulator, render
    assert D.MODES == ("fixed", "variance")   # a variance source of the variance mode, not a third mode
    assert D.MIN_MOMENT_BATCHES == 4
    assert inspect.signature(D.denoise_variance).parameters["variance"].default is None
    assert inspect.signature(D.denoise_variance_device).parameters["d_in_var_ptr"].default is None
    assert inspect.signature(D.moments_add).parameters["eps_a"].default == D.EPS_A
    assert inspect.signature(render).parameters["variance_batches"].default == 0
    assert inspect.signature(Accumulator.__init__).parameters["moments"].default is False
    assert callable(Accumulator.noise_map)


@pytest.mark.parametrize("kw,word", [
    (dict(spp=8, denoise="variance", variance_batches=3), "multiple"),
    (dict(spp=2, denoise="variance", variance_batches=4), "multiple"),
    (dict(spp=8, denoise="variance", variance_batches=4, devices=(0, 1)), "one device"),
    (dict(spp=8, denoise=True, variance_batches=4), "variance"),
    (dict(spp=8, denoise=False, variance_batches=4), "variance"),
    (dict(spp=8, denoise="variance", variance_batches=1), "variance_batches"),
    (dict(spp=8, denoise="variance", variance_batches=-2), "variance_batches"),
    (dict(spp=8, denoise="variance", variance_batches=2.0), "variance_batches"),
])
def test_render_rejects_bad_variance_batches(kw, word):
    from pyrenderer_amd.core.tracing import render
    with pytest.raises(ValueError, match=word):
        render(None, None, depth=1, **kw)


def test_accumulator_rejects_unequal_batches_before_it_renders():
    from pyrenderer_amd.core.tracing import Accumulator
    acc = object.__new__(Accumulator)   # no scene, no device: the check comes first
    acc.moments, acc.batch_spp, acc.samples = True, 2, 4
    with pytest.raises(ValueError, match="equal batches"):
        acc.add(3)
    assert acc.add(0) is acc and acc.samples == 4 and acc.batches == 2
    plain = object.__new__(Accumulator)
    plain.moments = False
    with pytest.raises(ValueError, match="moments=True"):
        plain.noise_map()


# ------------------------------------------------------------ command line ----

def test_variance_batches_flag():
    from pyrenderer_amd import main as M
    assert M.parse([]).variance_batches == 0
    a = M.parse(["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "4"])
    assert a.variance_batches == 4 and a.denoise and a.denoise_mode == "variance"
    b = M.parse(["--samples", "12", "--interval", "3", "--denoise", "--denoise-mode", "variance",
                 "--variance-batches", "5"])   # with --interval K only switches the moments on
    assert b.variance_batches == 5 and b.interval == 3
    c = M.parse(["--samples", "8", "--denoise-iterations", "3", "--denoise-mode", "variance", "--variance-batches", "2"])
    assert c.denoise and c.variance_batches == 2


@pytest.mark.parametrize("argv", [
    ["--samples", "8", "--variance-batches", "4"],                                             # no --denoise
    ["--samples", "8", "--denoise", "--variance-batches", "4"],                                # the fixed mode
    ["--samples", "8", "--denoise", "--denoise-mode", "fixed", "--variance-batches", "4"],
    ["--samples", "8", "--aov", "aov/", "--denoise-mode", "variance", "--variance-batches", "4"],
    ["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "1"],
    ["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "-4"],
    ["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "3"],   # 8 % 3
    ["--samples", "2", "--denoise", "--denoise-mode", "variance", "--variance-batches", "4"],
    ["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "x"],
    ["--samples", "8", "--denoise", "--denoise-mode", "variance", "--variance-batches", "4", "--devices", "0", "1"],
    ["--samples", "8", "--interval", "3", "--denoise", "--denoise-mode", "variance", "--variance-batches", "4"],
    ["--samples", "8", "--state", "acc", "--denoise", "--denoise-mode", "variance", "--variance-batches", "4"],
])
def test_variance_batches_usage_errors(argv, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.parse(argv)
    assert e.value.code == 2
    assert "--variance-batches" in capsys.readouterr().err

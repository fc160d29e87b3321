"""The temporal-accumulation entry points and their front ends without a GPU: declared, exported and bound;
bad arguments rejected before any device is touched, with the denoiser's own error text and the entry
point's name in front; the Python ValueErrors, the default signatures and the --frames / --orbit /
--temporal switches."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from temporal_abi_cases import FAKE, GOOD, ILLEGAL as _ILLEGAL, PARAM_NAMES, call as _call, cam as _cam

NAMES = ("prt_temporal_accumulate", "prt_temporal_accumulate_device", "prt_denoise_var_mixed",
         "prt_denoise_var_mixed_device")
VAR_GOOD = (1.0, 2.0, 1e-2, 1e-2, 1e-2)   # sigma_l, sigma_z, eps_a, eps_z, eps_l
VAR_PARAM_NAMES = ("sigma_l", "sigma_z", "eps_a", "eps_z", "eps_l")
# beside temporal_abi_cases.ILLEGAL: the edges of each range, which are legal
_LEGAL = {"alpha": (0.0, 1.0), "alpha_m": (0.0, 1.0), "tau_n": (-1.0, 1.0), "tau_a": (0.0,), "min_history": (1.0,),
          "w_min": (1.0,)}


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
    assert "#define PRT_TEMPORAL_CHANNELS 8" in src


def test_the_kernel_lives_in_an_auxiliary_unit_and_the_trace_kernels_key_is_unchanged():
    import json
    from pyrenderer_amd import build as B
    homes = [f for f in B.SOURCES + B.HEADERS + [B.TRACE_INST] + B.AUX_SOURCES + B.AUX_HEADERS
             if re.search(r"\btemporal_kernel\b|\bvar_estimate_kernel\b|\benqueue_temporal\b",
                          open(os.path.join(B.CSRC, f)).read())]
    assert homes and set(homes) <= set(B.AUX_SOURCES + B.AUX_HEADERS), homes
    assert not set(homes) & set(B.SOURCES + B.HEADERS + [B.TRACE_INST])
    src = open(os.path.join(B.CSRC, "prt_denoise.hip")).read()
    assert "temporal_kernel" in src
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', src)
    assert includes == ["prt_denoise.h"], includes          # no header of the trace kernels
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
    assert B.kernel_sha() in json.dumps(pmc)


# ------------------------------------------------------ prt_temporal_accumulate ----

_T_CASES = [("null_color", b"NULL"), ("null_feat", b"NULL"), ("null_cam", b"NULL"), ("null_state", b"NULL"),
            ("null_params", b"params8"), ("only_prev_feat", b"NULL together"), ("only_prev_cam", b"NULL together"),
            ("only_prev_state", b"NULL together"), ("no_prev_feat", b"NULL together"),
            ("no_prev_cam", b"NULL together"), ("no_prev_state", b"NULL together"),
            ("w0", b"W and H"), ("h0", b"W and H"), ("w_neg", b"W and H"), ("w_huge", b"W and H"),
            ("h_huge", b"W and H"), ("device_neg", b"device"), ("aperture", b"aperture"),
            ("prev_aperture", b"aperture"), ("cam_nan", b"camera record"), ("prev_cam_inf", b"camera record")]
_T_CASES += [(f"{name}:{how}", name.encode()) for name in PARAM_NAMES for how in _ILLEGAL[name]]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _T_CASES)
def test_temporal_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    from pyrenderer_amd import _native as N
    rc, msg, who, state = _call(N.lib(), N, device_form, case)
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(who) and word in msg, msg
    assert (state == 1).all()


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("name,value", [(n, v) for n, vs in _LEGAL.items() for v in vs])
def test_the_edges_of_the_ranges_are_legal(name, value, device_form):
    """A legal call passes every argument check and ends at the device ordinal, which is asked for last: one
    that no machine has is "no such device", or "no HIP device" without a GPU.  Nothing runs either way."""
    from pyrenderer_amd import _native as N
    rc, msg, who, _ = _call(N.lib(), N, device_form, f"legal={name}={value}")
    assert rc in (-1, -2) and msg.startswith(who) and (b"no such device" in msg or b"no HIP device" in msg), (rc, msg)


def test_temporal_device_form_checks_alignment_and_aliasing_without_a_gpu():
    from pyrenderer_amd import _native as N
    L = N.lib()
    par, cam, pcam = np.array(GOOD, np.float32), _cam(), _cam()
    pcam[3] = 0.25

    def dev(color=FAKE, feat=FAKE * 2, state=FAKE * 3, pfeat=FAKE * 4, pstate=FAKE * 5, out=None, var=None):
        rc = L.prt_temporal_accumulate_device(0, color, feat, N.ptr(cam), pfeat, N.ptr(pcam), pstate, 70, 130,
                                              N.ptr(par), state, out, var, None)
        return rc, L.prt_denoise_last_error()

    for kw in (dict(state=FAKE * 3 + 4), dict(pstate=FAKE * 5 + 8)):
        rc, msg = dev(**kw)
        assert rc == -1 and msg.startswith(b"prt_temporal_accumulate_device:") and b"aligned" in msg, msg
    for kw in (dict(state=FAKE * 5), dict(state=FAKE), dict(state=FAKE * 2), dict(state=FAKE * 4),
               dict(out=FAKE), dict(out=FAKE * 2), dict(out=FAKE * 4), dict(out=FAKE * 5), dict(out=FAKE * 3),
               dict(var=FAKE), dict(var=FAKE * 5), dict(var=FAKE * 3), dict(out=FAKE * 9, var=FAKE * 9)):
        rc, msg = dev(**kw)
        assert rc == -1 and msg.startswith(b"prt_temporal_accumulate_device:") and b"alias" in msg, (kw, msg)
    # the host form: the state in place of the previous state
    c, f, s = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32), np.zeros((2, 2, 8), np.float32)
    rc = L.prt_temporal_accumulate(0, N.ptr(c), N.ptr(f), N.ptr(cam), N.ptr(f), N.ptr(pcam), N.ptr(s), 2, 2,
                                   N.ptr(par), N.ptr(s), None, None)
    assert rc == -1 and b"prt_temporal_accumulate: state must not alias prev_state" in L.prt_denoise_last_error()


# ------------------------------------------------------ prt_denoise_var_mixed ----

_X_CASES = [("null_color", b"NULL"), ("null_feat", b"NULL"), ("null_in_var", b"NULL"), ("null_out", b"NULL"),
            ("null_params", b"NULL"), ("w0", b"W and H"), ("h0", b"W and H"), ("w_huge", b"W and H"),
            ("h_huge", b"W and H"), ("iter9", b"iterations"), ("iter_neg", b"iterations")]
_X_CASES += [(f"{name}:{how}", name.encode()) for name in VAR_PARAM_NAMES
             for how in ("0", "neg", "nan", "inf")]
_BAD_VALUES = {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf}


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _X_CASES)
def test_mixed_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H, it = 4, 3, 5
    color = np.zeros((W, H, 3), np.float32)
    feat = np.zeros((W, H, 8), np.float32)
    in_var = np.zeros((W, H), np.float32)
    out = np.zeros((W, H, 3), np.float32)
    par = np.array(VAR_GOOD, np.float32)
    if device_form:
        p = dict(color=FAKE, feat=FAKE * 2, in_var=FAKE * 3, out=FAKE * 4)
    else:
        p = dict(color=N.ptr(color), feat=N.ptr(feat), in_var=N.ptr(in_var), out=N.ptr(out))
    if case.startswith("null_") and case != "null_params":
        p[case[5:]] = None
    elif case == "null_params":
        par = None
    elif case in ("w0", "w_huge"):
        W = {"w0": 0, "w_huge": 32769}[case]
    elif case in ("h0", "h_huge"):
        H = {"h0": 0, "h_huge": 32769}[case]
    elif case in ("iter9", "iter_neg"):
        it = {"iter9": 9, "iter_neg": -1}[case]
    else:
        name, how = case.split(":")
        par[VAR_PARAM_NAMES.index(name)] = _BAD_VALUES[how]
    if device_form:
        rc = L.prt_denoise_var_mixed_device(0, p["color"], p["feat"], p["in_var"], W, H, it, N.ptr(par), p["out"], None,
                                            FAKE * 8, 1 << 40, None)
        who = b"prt_denoise_var_mixed_device:"
    else:
        rc = L.prt_denoise_var_mixed(0, p["color"], p["feat"], p["in_var"], W, H, it, N.ptr(par), p["out"], None)
        who = b"prt_denoise_var_mixed:"
    msg = L.prt_denoise_last_error()
    assert rc == -1, (rc, msg)
    assert msg.startswith(who) and word in msg, msg


def test_mixed_device_form_checks_scratch_and_aliasing_without_a_gpu():
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H = 70, 130
    need = L.prt_denoise_var_work_bytes(W, H)   # no new scratch: the estimate's kernel selects as it writes its planes
    par = np.array(VAR_GOOD, np.float32)

    def dev(color=FAKE, in_var=FAKE * 7, out=FAKE * 2, var=None, work=FAKE * 3, size=need):
        rc = L.prt_denoise_var_mixed_device(0, color, FAKE * 5, in_var, W, H, 5, N.ptr(par), out, var, work, size, None)
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
        assert rc == -1 and b"alias" in msg and b"d_out_var" in msg and msg.startswith(b"prt_denoise_var_mixed_device:")


# ------------------------------------------------------------------ Python ----

def test_python_wrappers_raise():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd import denoise as D
    c, f, cam = np.zeros((2, 2, 3), np.float32), np.zeros((2, 2, 8), np.float32), _cam()
    st = D.temporal_state(2, 2)
    assert st.shape == (2, 2, 8) and st.dtype == np.float32 and not st.any() and D.TEMPORAL_CHANNELS == 8
    with pytest.raises(ValueError, match="aperture"):
        D.temporal_accumulate(c, f, _cam(0.2))
    with pytest.raises(ValueError, match="aperture"):
        D.temporal_accumulate(c, f, cam, (st, f, _cam(0.2)))
    with pytest.raises(ValueError, match="24 floats"):
        D.temporal_accumulate(c, f, cam[:20])
    with pytest.raises(ValueError, match="resolution cannot change"):
        D.temporal_accumulate(c, f, cam, (D.temporal_state(2, 3), np.zeros((2, 3, 8), np.float32), cam))
    with pytest.raises(ValueError, match="feat must be"):
        D.temporal_accumulate(c, np.zeros((2, 2, 7), np.float32), cam)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate: tau_z"):
        D.temporal_accumulate(c, f, cam, tau_z=0.0)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate: w_min"):
        D.temporal_accumulate(c, f, cam, (st, f, cam), w_min=np.nan)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_device: alpha"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, alpha=2.0)
    with pytest.raises(N.PrtError, match="prt_temporal_accumulate_device: .*NULL together"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, cam, 2, 2, FAKE * 3, prev_cam=cam)
    with pytest.raises(ValueError, match="aperture"):
        D.temporal_accumulate_device(FAKE, FAKE * 2, _cam(1.0), 2, 2, FAKE * 3)
    with pytest.raises(ValueError, match="variance_fallback"):
        D.denoise_variance(c, f, variance=np.zeros((2, 2), np.float32), variance_fallback="temporal")
    with pytest.raises(ValueError, match="needs a variance plane"):
        D.denoise_variance(c, f, variance_fallback="spatial")
    with pytest.raises(ValueError, match="needs a variance plane"):
        D.denoise_variance_device(FAKE, FAKE * 2, 2, 2, FAKE * 3, FAKE * 4, 1 << 20, variance_fallback="spatial")
    with pytest.raises(N.PrtError, match="prt_denoise_var_mixed: iterations"):
        D.denoise_variance(c, f, iterations=9, variance=np.zeros((2, 2), np.float32), variance_fallback="spatial")
    with pytest.raises(N.PrtError, match="prt_denoise_var_mixed_device: iterations"):
        D.denoise_variance_device(FAKE, FAKE * 2, 2, 2, FAKE * 3, FAKE * 4, 1 << 20, iterations=9,
                                  d_in_var_ptr=FAKE * 5, variance_fallback="spatial")
    with pytest.raises(N.PrtError, match="prt_denoise_var_given: iterations"):   # "zero" is today's path
        D.denoise_variance(c, f, iterations=9, variance=np.zeros((2, 2), np.float32))


def test_constants_and_signatures():
    from pyrenderer_amd import denoise as D
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    assert D.MODES == ("fixed", "variance")   # a source of colour and variance for the variance mode
    sig = inspect.signature(D.temporal_accumulate).parameters
    assert sig["prev"].default is None and sig["return_color"].default is True and sig["device"].default == 0
    assert tuple(n for n in sig if n in PARAM_NAMES) == PARAM_NAMES == D.TEMPORAL_PARAMS
    for name, const in zip(PARAM_NAMES, (D.TEMPORAL_ALPHA, D.TEMPORAL_ALPHA_M, D.TEMPORAL_TAU_N, D.TEMPORAL_TAU_Z,
                                         D.TEMPORAL_TAU_A, D.EPS_A, D.TEMPORAL_MIN_HISTORY, D.TEMPORAL_W_MIN)):
        assert sig[name].default == const, name
        assert inspect.signature(D.temporal_accumulate_device).parameters[name].default == const, name
    assert inspect.signature(D.denoise_variance).parameters["variance_fallback"].default == "zero"
    assert inspect.signature(D.denoise_variance_device).parameters["variance_fallback"].default == "zero"
    sig = inspect.signature(TemporalAccumulator.__init__).parameters
    assert sig["seed"].default == 0 and sig["device"].default == 0 and sig["tile"].default == 64
    assert sig["world"].default is None and sig["nee"].default == "reference"
    for m in ("add", "mean", "accumulated", "history", "denoised", "reset"):
        assert callable(getattr(TemporalAccumulator, m)), m
    assert inspect.signature(render_sequence).parameters["denoise"].default == "variance"


def test_temporal_accumulator_rejects_before_it_renders():
    from pyrenderer_amd.core.camera import Camera, orbit
    from pyrenderer_amd.core.tracing import TemporalAccumulator, render_sequence
    lens = Camera((0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 8), aperture=0.1)
    acc = TemporalAccumulator(None, depth=2, spp=1)          # no scene, no device: the checks come first
    with pytest.raises(ValueError, match="pinhole"):
        acc.add(lens)
    with pytest.raises(ValueError, match="add\\(camera\\) first"):
        acc.accumulated()
    acc.resolution = (8, 8)                                   # as after a first camera of 8 x 8
    with pytest.raises(ValueError, match="resolution cannot change"):
        acc.add(Camera((0, 0, 4), (0, 0, 0), (0, 1, 0), (8, 9)))
    with pytest.raises(TypeError, match="sigma_l"):
        TemporalAccumulator(None, depth=2, spp=1, sigma_l=1.0)
    with pytest.raises(ValueError, match="spp"):
        TemporalAccumulator(None, depth=2, spp=0)
    with pytest.raises(ValueError, match="nee"):
        TemporalAccumulator(None, depth=2, spp=1, nee="both")
    with pytest.raises(ValueError, match="denoise must be"):
        render_sequence(None, [lens], spp=1, depth=2, denoise=True)
    with pytest.raises(ValueError, match="at least one camera"):
        render_sequence(None, [], spp=1, depth=2)
    with pytest.raises(ValueError, match="pinhole"):
        render_sequence(None, [lens], spp=1, depth=2)
    # orbit: a turn about the look-at point around the up vector keeps distance and height
    cam = Camera((3.0, 1.0, 4.0), (0.5, 1.0, 0.0), (0, 1, 0), (8, 8), fov=40)
    turned = orbit(cam, 90.0)
    assert np.allclose(turned.position, (0.5 + 4.0, 1.0, 0.0 - 2.5)) and turned.fov == 40
    assert np.allclose(orbit(turned, -90.0).position, cam.position)
    assert np.array_equal(orbit(cam, 0.0).packed(), cam.packed())


# ------------------------------------------------------------ command line ----

def test_frames_flags():
    from pyrenderer_amd import main as M
    a = M.parse([])
    assert a.frames == 0 and a.orbit == 0.0 and a.temporal is False
    a = M.parse(["--samples", "2", "--frames", "8", "--orbit", "2", "--temporal", "--denoise", "--denoise-mode",
                 "variance"])
    assert a.frames == 8 and a.orbit == 2.0 and a.temporal and a.denoise_mode == "variance"
    a = M.parse(["--samples", "1", "--frames", "3", "--orbit", "-1.5", "--temporal"])   # no --denoise at all
    assert a.temporal and not a.denoise and a.orbit == -1.5
    a = M.parse(["--frames", "3", "--orbit", "5", "--denoise"])                          # no history: any mode
    assert a.frames == 3 and not a.temporal
    assert M.frame_path("out.png", 7) == "out.0007.png" and M.frame_path("a/b.c/img", 12) == "a/b.c/img.0012"


@pytest.mark.parametrize("argv,flag", [
    (["--temporal"], "--temporal"),
    (["--orbit", "2"], "--orbit"),
    (["--frames", "-1"], "--frames"),
    (["--frames", "x"], "--frames"),
    (["--frames", "4", "--samples", "0"], "--samples"),
    (["--frames", "4", "--temporal", "--denoise"], "--temporal"),                        # the fixed mode
    (["--frames", "4", "--temporal", "--denoise", "--denoise-mode", "fixed"], "--temporal"),
    (["--frames", "4", "--temporal", "--denoise-iterations", "3"], "--temporal"),
    (["--frames", "4", "--temporal", "--interval", "2"], "--interval"),
    (["--frames", "4", "--temporal", "--state", "acc"], "--state"),
    (["--frames", "4", "--temporal", "--hdr", "hdr/"], "--hdr"),
    (["--frames", "4", "--temporal", "--devices", "0", "1"], "--devices"),
    (["--frames", "4", "--temporal", "--samples", "8", "--denoise", "--denoise-mode", "variance",
      "--variance-batches", "4"], "--variance-batches"),
    (["--frames", "4", "--interval", "2"], "--interval"),
])
def test_frames_usage_errors(argv, flag, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.parse(argv)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err

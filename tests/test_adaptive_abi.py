"""The adaptive-sampling entry points and their front ends without a GPU: declared, exported and bound; the
kernel where it belongs; the trace kernels' key untouched; bad arguments rejected before any device is touched,
with the denoiser's own error text; the Python ValueErrors and the command line's conflicts."""
import glob
import inspect
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("prt_adaptive_update", "prt_adaptive_update_device")
FAKE = 4096   # a device "pointer" that is never dereferenced: the checks fail first
_BAD_VALUES = {"0": 0.0, "neg": -1.0, "nan": np.nan, "inf": np.inf}


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
    assert "prt_adaptive_update*" in src[src.index("ABI history"):src.index("#define PRT_ABI_VERSION")]


def test_the_kernel_lives_in_the_denoiser_unit_and_the_trace_key_is_unchanged():
    from pyrenderer_amd import build as B
    csrc = os.path.join(ROOT, "pyrenderer_amd", "csrc")
    holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*"))
                     if "adaptive_kernel" in open(p, errors="replace").read())
    assert holders == ["prt_denoise.h", "prt_denoise.hip"] or holders == ["prt_denoise.hip"], holders
    hip = open(os.path.join(csrc, "prt_denoise.hip")).read()
    assert re.findall(r"^\s*#\s*include\s+(\S+)", hip, re.M) == ['"prt_denoise.h"']
    assert len(re.findall(r"__global__[^;{]*\badaptive_kernel\b", hip)) == 1
    # the update is moments_kernel's own: both kernels call the shared steps, neither restates them
    for step in ("welford_add(", "variance_of_mean(", "batch_luminance("):
        assert hip.count(step) == 3, step   # the definition and the two kernels
    assert set(B.AUX_SOURCES) == {"prt_denoise.hip", "prt_denoise_capi.cpp"} and B.AUX_HEADERS == ["prt_denoise.h"]
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc.json")))
    assert B.kernel_sha() in json.dumps(pmc)


# ------------------------------------------------------------ bad arguments ----

_CASES = [(f"null_{n}", b"NULL") for n in ("batch", "ids", "feat", "params", "sum", "state", "records")]
_CASES += [("w0", b"W and H"), ("h0", b"W and H"), ("w_huge", b"W and H"), ("h_huge", b"W and H"),
           ("tw3", b"powers of two"), ("th12", b"powers of two"), ("tw0", b"powers of two"), ("tile_small", b"64..2^20"),
           ("tile_huge", b"64..2^20"), ("id_high", b"out of range"), ("id_neg", b"out of range"),
           ("id_twice", b"twice"), ("n_tiles_neg", b"n_tiles"), ("slots", b"2^31"),
           ("n0", b"n_samples"), ("n_half", b"n_samples"), ("n_nan", b"n_samples"), ("n_inf", b"n_samples"),
           ("target_nan", b"target"), ("target_neg", b"target")]
_CASES += [(f"{name}:{how}", name.encode()) for name in ("eps_a", "eps_r") for how in _BAD_VALUES]


def _call(device_form, case="ok", ids=(0, 1, 2, 3)):
    """One call on a 13 x 9 frame of four 8 x 8 tiles with `case` wrong: (rc, message, the host arrays)."""
    from pyrenderer_amd import _native as N
    L = N.lib()
    W, H, tw, th, n, eps_a = 13, 9, 8, 8, 4.0, 1e-2
    ids = np.array(ids, np.int32)
    n_tiles = len(ids)
    par = np.array([1e-3, 0.05], np.float32)
    host = dict(batch=np.zeros((max(n_tiles, 1) * 64, 3), np.float32), feat=np.zeros((W, H, 8), np.float32),
                sum=np.zeros((W, H, 3), np.float32), state=np.zeros((W, H, 4), np.float32),
                records=np.zeros((max(n_tiles, 1), 4), np.uint32))
    if device_form:
        p = {k: FAKE * 16 * (j + 1) for j, k in enumerate(host)}
    else:
        p = {k: N.ptr(v) for k, v in host.items()}
    p["ids"], p["params"] = N.ptr(ids), N.ptr(par)
    if case.startswith("null_"):
        p[case[5:]] = None
    elif case in ("w0", "h0", "w_huge", "h_huge"):
        W, H = {"w0": (0, H), "h0": (W, 0), "w_huge": (32769, H), "h_huge": (W, 32769)}[case]
    elif case in ("tw3", "th12", "tw0", "tile_small", "tile_huge"):
        tw, th = {"tw3": (3, 32), "th12": (8, 12), "tw0": (0, 64), "tile_small": (8, 4), "tile_huge": (2048, 1024)}[case]
    elif case == "id_high":
        ids[2] = 4
    elif case == "id_neg":
        ids[1] = -1
    elif case == "id_twice":
        ids[3] = ids[0]
    elif case == "n_tiles_neg":
        n_tiles = -1
    elif case == "slots":
        n_tiles = (1 << 31) // 64   # the list is not read: the count fails first
    elif case in ("n0", "n_half", "n_nan", "n_inf"):
        n = {"n0": 0.0, "n_half": 0.5, "n_nan": np.nan, "n_inf": np.inf}[case]
    elif case == "target_nan":
        par[1] = np.nan
    elif case == "target_neg":
        par[1] = -0.5
    elif ":" in case:
        name, how = case.split(":")
        if name == "eps_a":
            eps_a = _BAD_VALUES[how]
        else:
            par[0] = _BAD_VALUES[how]
    args = [0, p["batch"], p["ids"], n_tiles, tw, th, W, H, p["feat"], eps_a, n, p["params"], p["sum"], p["state"],
            p["records"]]
    rc = L.prt_adaptive_update_device(*args, None) if device_form else L.prt_adaptive_update(*args)
    return rc, L.prt_denoise_last_error(), host


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("case,word", _CASES)
def test_bad_arguments_are_rejected_before_any_device(case, word, device_form):
    rc, msg, host = _call(device_form, case)
    who = b"prt_adaptive_update_device:" if device_form else b"prt_adaptive_update:"
    assert rc == -1, (rc, msg)   # PRT_ERR_ARG
    assert msg.startswith(who) and word in msg, msg
    assert not any(a.any() for a in host.values())


@pytest.mark.parametrize("device_form", [False, True])
def test_an_empty_list_is_ok_and_touches_nothing(device_form):
    from pyrenderer_amd import _native as N
    L = N.lib()
    rc, msg, host = _call(device_form, ids=())
    assert rc == 0, msg
    assert not any(a.any() for a in host.values())
    par = np.array([1e-3, np.inf], np.float32)   # +inf is a legal target, and no pointer is looked at
    fn = L.prt_adaptive_update_device if device_form else L.prt_adaptive_update
    assert fn(0, None, None, 0, 8, 8, 13, 9, None, 1e-2, 4.0, N.ptr(par), None, None, None, *([None] * device_form)) == 0
    # ... but the shape and the parameters are still checked
    assert fn(0, None, None, 0, 8, 8, 0, 9, None, 1e-2, 4.0, N.ptr(par), None, None, None, *([None] * device_form)) == -1
    assert fn(0, None, None, 0, 8, 8, 13, 9, None, 1e-2, 4.0, None, None, None, None, *([None] * device_form)) == -1


def test_device_form_wants_an_aligned_state():
    from pyrenderer_amd import _native as N
    L = N.lib()
    ids, par = np.array([0], np.int32), np.array([1e-3, 0.05], np.float32)
    rc = L.prt_adaptive_update_device(0, FAKE, N.ptr(ids), 1, 8, 8, 13, 9, FAKE * 2, 1e-2, 4.0, N.ptr(par), FAKE * 3,
                                      FAKE * 4 + 4, FAKE * 5, None)
    msg = L.prt_denoise_last_error()
    assert rc == -1 and b"aligned" in msg and b"d_io_state" in msg, msg


# ------------------------------------------------------------------ Python ----

def test_signatures_and_lazy_import():
    from pyrenderer_amd import adaptive as A
    from pyrenderer_amd.core import tracing as T
    p = inspect.signature(A.AdaptiveAccumulator.__init__).parameters
    assert list(p)[:3] == ["self", "scene", "camera"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])
    assert p["min_batches"].default == 2 and p["tolerate"].default == 0.0 and p["tile"].default == 64
    assert p["seed"].default == 0 and p["nee"].default == "reference" and p["eps_r"].default == A.EPS_R > 0
    for name in ("step", "run", "samples", "sums", "mean", "moments", "noise_map", "records", "features", "denoised"):
        assert callable(getattr(A.AdaptiveAccumulator, name)), name
    r = inspect.signature(T.render_adaptive).parameters
    assert r["denoise"].default is False and r["return_samples"].default is False
    assert inspect.signature(T._Frame.add_samples).parameters["ids"].default is None
    # core/tracing.py imports the module inside render_adaptive only
    src = open(os.path.join(ROOT, "pyrenderer_amd", "core", "tracing.py")).read()
    assert not re.search(r"^(from|import)\b.*\b(adaptive|torch)\b", src, re.M)


@pytest.mark.parametrize("kw,word", [
    (dict(batch_spp=0), "batch_spp"), (dict(batch_spp=2.0), "batch_spp"), (dict(batch_spp=True), "batch_spp"),
    (dict(target=-1.0), "target"), (dict(target=np.nan), "target"), (dict(min_batches=1), "min_batches"),
    (dict(min_batches=2.5), "min_batches"), (dict(tolerate=1.0), "tolerate"), (dict(tolerate=-0.01), "tolerate"),
    (dict(eps_r=0.0), "eps_r"), (dict(eps_r=np.inf), "eps_r")])
def test_the_sampler_rejects_bad_parameters_before_it_touches_a_scene(kw, word):
    from pyrenderer_amd.adaptive import AdaptiveAccumulator
    from pyrenderer_amd.core.tracing import render_adaptive
    args = dict(depth=4, batch_spp=4, target=0.05)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        AdaptiveAccumulator(None, None, **args)
    with pytest.raises(ValueError, match=word):
        render_adaptive(None, None, max_batches=4, **args)


@pytest.mark.parametrize("kw,word", [(dict(max_batches=0), "max_batches"), (dict(max_batches=2.0), "max_batches"),
                                     (dict(max_batches=4, denoise="fixed"), "denoise")])
def test_render_adaptive_rejects_its_own_bad_arguments(kw, word):
    from pyrenderer_amd.core.tracing import render_adaptive
    with pytest.raises(ValueError, match=word):
        render_adaptive(None, None, depth=4, batch_spp=4, target=0.05, **kw)


def test_host_wrapper_raises():
    from pyrenderer_amd import _native as N
    from pyrenderer_amd.adaptive import adaptive_update, adaptive_update_device
    s, st, f = np.zeros((13, 9, 3), np.float32), np.zeros((13, 9, 4), np.float32), np.zeros((13, 9, 8), np.float32)
    b = np.zeros((2 * 64, 3), np.float32)
    with pytest.raises(ValueError, match="io_state"):
        adaptive_update(s, st.astype(np.float64), b, [0, 1], 8, 8, f, 4, target=0.1)
    with pytest.raises(ValueError, match="batch"):
        adaptive_update(s, st, b[:-1], [0, 1], 8, 8, f, 4, target=0.1)
    with pytest.raises(ValueError, match="feat"):
        adaptive_update(s, st, b, [0, 1], 8, 8, f[..., :7], 4, target=0.1)
    with pytest.raises(N.PrtError, match="prt_adaptive_update: tile id listed twice: 1"):
        adaptive_update(s, st, b, [1, 1], 8, 8, f, 4, target=0.1)
    with pytest.raises(N.PrtError, match="prt_adaptive_update_device: target"):
        adaptive_update_device(FAKE, [0], 8, 8, 13, 9, FAKE * 2, 4, FAKE * 3, FAKE * 4, FAKE * 5, target=-1.0)


# ------------------------------------------------------------ command line ----

def test_adaptive_flags():
    from pyrenderer_amd import main as M
    a = M.parse([])
    assert a.adaptive is None and a.batch_spp is None and a.max_samples is None
    b = M.parse(["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "256"])
    assert b.adaptive == 0.05 and b.batch_spp == 8 and b.max_samples == 256 and b.min_batches == 2 and b.tolerate == 0.0
    c = M.parse(["--adaptive", "0", "--batch-spp", "4", "--max-samples", "16", "--min-batches", "3", "--tolerate", "0.02",
                 "--denoise", "--denoise-mode", "variance", "--aov", "aov/"])
    assert c.adaptive == 0.0 and c.min_batches == 3 and c.tolerate == 0.02 and c.denoise


@pytest.mark.parametrize("argv", [
    ["--batch-spp", "8"], ["--max-samples", "64"], ["--min-batches", "3"], ["--tolerate", "0.1"],   # no --adaptive
    ["--adaptive", "0.05"], ["--adaptive", "0.05", "--batch-spp", "8"], ["--adaptive", "0.05", "--max-samples", "64"],
    ["--adaptive", "-1", "--batch-spp", "8", "--max-samples", "64"],
    ["--adaptive", "nan", "--batch-spp", "8", "--max-samples", "64"],
    ["--adaptive", "0.05", "--batch-spp", "0", "--max-samples", "64"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "60"],     # no multiple
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "4"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--min-batches", "1"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--tolerate", "1"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--devices", "0", "1"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--interval", "8"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--denoise", "--denoise-mode", "variance",
     "--variance-batches", "4"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--frames", "2", "--temporal"],
    ["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64", "--state", "acc"],
])
def test_adaptive_usage_errors(argv, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit) as e:
        M.parse(argv)
    assert e.value.code == 2
    assert "--adaptive" in capsys.readouterr().err


@pytest.mark.parametrize("flag,argv", [("--devices", ["--devices", "0", "1"]), ("--interval", ["--interval", "8"]),
                                       ("--variance-batches", ["--denoise", "--denoise-mode", "variance",
                                                               "--variance-batches", "4"]),
                                       ("--temporal", ["--frames", "2", "--temporal"])])
def test_a_conflict_names_the_switch(flag, argv, capsys):
    from pyrenderer_amd import main as M
    with pytest.raises(SystemExit):
        M.parse(["--adaptive", "0.05", "--batch-spp", "8", "--max-samples", "64"] + argv)
    err = capsys.readouterr().err
    assert "cannot be combined with" in err and flag in err

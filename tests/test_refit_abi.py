"""prt_scene_update and prt_scene_download: declared in include/prt.h and bound in _native.py under ABI 4 with
their lines in the header's history, both refuse a NULL scene without a device, and the host half of an
update (argument checks, level lists, the pad rule) runs clean under AddressSanitizer and UBSan in a
stand-alone driver (tools/sanitize/refit_check.cpp)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "prt.h")).read()


def test_declared_and_bound():
    from pyrenderer_amd import _native as N
    src = header()
    for name in ("prt_scene_update", "prt_scene_download"):
        assert re.search(r"^int %s\(" % name, src, re.M) and name in N.EXPORTS, name
    assert "#define PRT_ABI_VERSION 4" in src and N.ABI_VERSION == 4
    history = src[src.index("ABI history"):src.index("#define PRT_ABI_VERSION")]
    assert "prt_scene_update" in history and "prt_scene_download" in history
    consts = {k: int(v, 0) for k, v in re.findall(r"^#define\s+(PRT_BUF_[A-Z0-9_]+)\s+(\w+)", src, re.M)}
    assert len(consts) == 10 and consts == {k: v for k, v in vars(N).items() if k.startswith("PRT_BUF_")}
    from pyrenderer_amd import build as B
    assert "prt_refit.hip" in B.SOURCES


def test_null_scene_is_an_argument_error_without_a_device():
    from pyrenderer_amd import _native as N
    L = N.lib()
    assert L.prt_abi_version() == 4
    v = np.zeros(9, np.float32)
    assert L.prt_scene_update(None, N.ptr(v), N.ptr(v), None) == N.PRT_ERR_ARG
    assert b"NULL" in L.prt_last_error()
    out = np.zeros(4, np.int64)
    assert L.prt_scene_download(None, N.PRT_BUF_NODES4, N.ptr(out), out.nbytes) == N.PRT_ERR_ARG
    assert L.prt_scene_download(None, N.PRT_BUF_NODES4 | N.PRT_BUF_BYTES, N.ptr(out), 8) == N.PRT_ERR_ARG


def _sanitizer_runtime():
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        return False
    r = subprocess.run([cxx, "-print-file-name=libasan.so"], capture_output=True, text=True)
    return r.returncode == 0 and os.path.isabs(r.stdout.strip())


@pytest.mark.skipif(not _sanitizer_runtime(), reason="no AddressSanitizer runtime for g++")
@pytest.mark.parametrize("n,seed", [(1, 1), (3000, 3), (20000, 7)])
def test_host_half_clean_under_asan_ubsan(n, seed):
    san = os.path.join(ROOT, "tools", "sanitize")
    exe = os.path.join(ROOT, "build", "sanitize", "refit_check")
    subprocess.run(["make", "-s", "-C", san, exe], check=True, capture_output=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(n), str(seed)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["failures"] == 0 and rep["refused"] == 7 and rep["triangles"] == n, rep
    assert rep["references"] >= n and rep["levels4"] >= rep["levels8"] >= 1, rep


def test_refit_flag_needs_a_spin(capsys):
    from pyrenderer_amd.main import parse
    for argv in (["--frames", "2", "--refit"], ["--refit"]):
        with pytest.raises(SystemExit):
            parse(argv)
    assert "--spin" in capsys.readouterr().err
    assert parse(["--frames", "2", "--spin", "5", "6", "--refit"]).refit
    assert not parse(["--frames", "2", "--spin", "5", "6"]).refit

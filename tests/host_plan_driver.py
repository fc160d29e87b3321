"""The stand-alone driver of libprt's host arithmetic (tools/sanitize/host_check.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer): the fixture that builds it, one call of it, and a scene
handed to its `scene` command.  Used by tests/test_host_plan.py and tests/test_shade_cases.py.  A
subprocess per call: exit code 0, no sanitizer text on stderr, one JSON line on stdout."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scene_cases import ARRAYS

SAN = os.path.join(ROOT, "tools", "sanitize")
OUT = os.path.join(ROOT, "build", "sanitize")
F = np.float32


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-s", "-C", SAN, os.path.join(OUT, "host_check")], check=True, capture_output=True,
                   timeout=600)
    return os.path.join(OUT, "host_check")


def _run(built, *args, **env):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1", **env)
    r = subprocess.run([built] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _scene(built, d, s):
    os.makedirs(d, exist_ok=True)
    for name in ARRAYS:
        if s[name] is not None:
            np.ascontiguousarray(s[name]).tofile(os.path.join(d, name + (".f32" if s[name].dtype == F else ".i32")))
    return _run(built, "scene", d, s["n_tri"], s["n_sph"], s["n_mat"], s["n_light"])


def _flat_args(flat):
    has_sph = flat.sph.shape[0] > 0
    return dict(tri_v=flat.tri_v, tri_n=flat.tri_n, tri_mat=flat.tri_mat, n_tri=flat.n_tri,
                sph=flat.sph if has_sph else None, sph_mat=flat.sph_mat if has_sph else None, n_sph=flat.sph.shape[0],
                mat=flat.mat, n_mat=flat.mat.shape[0], light_tri=flat.light_tri, light_off=flat.light_off,
                n_light=flat.n_light)
